// Reflection probes (mcpt.h: reflection probes): the arithmetic of a probe's octahedral radiance map -- a direction's place in the unit
// square and back, a texel's centre direction and solid angle, the wrap of a tap across the square's seams, the integer power of a Phong
// lobe -- of the prefilter that convolves a map with such lobes and of the lookup in the chain of filtered maps, the one copy of it:
// reflection.hip compiles it for the GPU, reflection_api.cpp for mcpt_reflection_texels, mcpt_reflection_prefilter_host and
// mcpt_reflection_lookup_host.  fp64, no contraction (-ffp-contract=off), IEEE division, every expression in the order mcpt.h writes it;
// tests/reflection_ref.py restates it in numpy.  The launch interface of the kernels is at the end.
#pragma once
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mcpt.h"
#include "visibility.hpp"

namespace mcpt {

constexpr int32_t kReflectionMaxRes = 256;       // texels per side of a map or a level
constexpr int32_t kReflectionMaxLevels = 8;
constexpr int32_t kReflectionMaxNs = 65535;      // the largest exponent of a level

// the fold of the lower hemisphere (z < 0) over the square's diagonals, from the old u and v: mcpt_visibility_bin's
MCPT_HD void reflection_fold(double& u, double& v)
{
    const double u0 = u, v0 = v;
    u = (1.0 - fabs(v0)) * (u0 >= 0.0 ? 1.0 : -1.0);
    v = (1.0 - fabs(u0)) * (v0 >= 0.0 ? 1.0 : -1.0);
}

// (s, t) in [0, 1]^2 of direction (x, y, z) of any non-zero finite length.  A direction that is zero or not finite gives NaN (the
// host-pointer forms refuse it first; the lookup's clamp takes a NaN to the border).
MCPT_HD void reflection_encode(double x, double y, double z, double& s, double& t)
{
    const double l = (fabs(x) + fabs(y)) + fabs(z);
    double u = x / l, v = y / l;
    if (z < 0.0) reflection_fold(u, v);
    s = u * 0.5 + 0.5;
    t = v * 0.5 + 0.5;
}

// the folded, unnormalised (u, v, z) of the point (s, t) of the square
MCPT_HD void reflection_square(double s, double t, double& u, double& v, double& z)
{
    u = 2.0 * s - 1.0;
    v = 2.0 * t - 1.0;
    z = (1.0 - fabs(u)) - fabs(v);
    if (z < 0.0) reflection_fold(u, v);
}

// the unit direction of the point (s, t) of the square
MCPT_HD void reflection_decode(double s, double t, double* d)
{
    double u, v, z;
    reflection_square(s, t, u, v, z);
    const double l = sqrt((u * u + v * v) + z * z);
    d[0] = u / l; d[1] = v / l; d[2] = z / l;
}

// Texel b = y * R + x of an R x R map: the direction of its centre ((x + 0.5) / R, (y + 0.5) / R) and its midpoint-rule solid angle
// du dv / |p|^3 with p the centre's folded, unnormalised (u, v, z)
MCPT_HD void reflection_texel(int R, int b, double* d, double& w)
{
    const int x = b % R, y = b / R;
    double u, v, z;
    reflection_square((double(x) + 0.5) / double(R), (double(y) + 0.5) / double(R), u, v, z);
    const double n2 = (u * u + v * v) + z * z, l = sqrt(n2);
    d[0] = u / l; d[1] = v / l; d[2] = z / l;
    w = ((2.0 / double(R)) * (2.0 / double(R))) / (n2 * l);
}

// A tap (x, y), x and y in -1 .. R, taken across the square's edges -- all four are seams of the lower hemisphere -- into 0 .. R - 1
MCPT_HD void reflection_wrap(int R, int& x, int& y)
{
    if (x < 0 || x >= R) {
        x = x < 0 ? -1 - x : 2 * R - 1 - x;
        y = R - 1 - y;
    }
    if (y < 0 || y >= R) {
        y = y < 0 ? -1 - y : 2 * R - 1 - y;
        x = R - 1 - x;
    }
}

// c^n for an integer n >= 0 by binary squaring, in the order mcpt.h writes: no pow, so numpy restates it bit for bit
MCPT_HD double reflection_ipow(double c, int n)
{
    double r = 1.0, b = c;
    while (n > 0) {
        if (n & 1) r = r * b;
        n >>= 1;
        if (n) b = b * b;
    }
    return r;
}

// One output texel of the prefilter: the map L [texels][3] of a probe, whose texel b has direction dw[b * 4 .. + 3) and solid angle
// dw[b * 4 + 3], under the lobe cos^ns about r, summed over the source in ascending order.  An empty lobe (W == 0) gives +0.0.
MCPT_HD void reflection_filter(const double* dw, const double* L, int texels, const double* r, int ns, double* out)
{
    double W = 0.0, A[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < texels; b++) {
        const double* e = dw + size_t(b) * 4;
        const double c = (r[0] * e[0] + r[1] * e[1]) + r[2] * e[2];
        if (c > 0.0) {
            const double g = e[3] * reflection_ipow(c, ns);
            W += g;
            for (int ch = 0; ch < 3; ch++) A[ch] += g * L[size_t(b) * 3 + size_t(ch)];
        }
    }
    for (int ch = 0; ch < 3; ch++) out[ch] = W > 0.0 ? A[ch] / W : 0.0;
}

// texels of a chain: the sum of its levels' squares (a checked chain: at most 8 * 65 536)
MCPT_HD int reflection_chain_texels(const mcpt_reflection_chain& c)
{
    int t = 0;
    for (int l = 0; l < c.num_levels; l++) t += c.level_res[l] * c.level_res[l];
    return t;
}

// One axis of a lookup inside a level: tap i0 in -1 .. R - 1 and the fraction towards i0 + 1.  The clamp is in double, before any
// conversion to int; a NaN takes -1 (lightmap_span's rule), never a tap outside -1 .. R.  s in [0, 1] gives -0.5 .. R - 0.5 by itself:
// half a texel beyond either border, where the tap across the seam weighs as much as the border's own -- a clamp at R - 1 would cut
// that blend at the high borders and the lookup would jump across those seams.
MCPT_HD void reflection_axis(double s, int R, int& i0, double& f)
{
    const double top = double(R) - 0.5;
    double a = s * double(R) - 0.5;
    a = a > -1.0 ? a : -1.0;
    a = a < top ? a : top;
    const double fl = floor(a);
    i0 = int(fl);
    f = a - fl;
}

// the bilinear value of direction d in the level m [R * R][3]
MCPT_HD void reflection_level(const double* m, int R, const double* d, double* v)
{
    double s, t, fx, fy;
    reflection_encode(d[0], d[1], d[2], s, t);
    int x0, y0;
    reflection_axis(s, R, x0, fx);
    reflection_axis(t, R, y0, fy);
    int tx[4] = {x0, x0 + 1, x0, x0 + 1}, ty[4] = {y0, y0, y0 + 1, y0 + 1};
    for (int j = 0; j < 4; j++) reflection_wrap(R, tx[j], ty[j]);
    const double w00 = (1.0 - fx) * (1.0 - fy), w10 = fx * (1.0 - fy), w01 = (1.0 - fx) * fy, w11 = fx * fy;
    const double* m00 = m + (size_t(ty[0]) * size_t(R) + size_t(tx[0])) * 3;
    const double* m10 = m + (size_t(ty[1]) * size_t(R) + size_t(tx[1])) * 3;
    const double* m01 = m + (size_t(ty[2]) * size_t(R) + size_t(tx[2])) * 3;
    const double* m11 = m + (size_t(ty[3]) * size_t(R) + size_t(tx[3])) * 3;
    for (int ch = 0; ch < 3; ch++) v[ch] = ((w00 * m00[ch] + w10 * m10[ch]) + w01 * m01[ch]) + w11 * m11[ch];
}

MCPT_HD double reflection_wt(double a) { return 1.0 / sqrt(a + 1.0); }

// The lookup of one receiver in the chain p [T][3] of its probe: the level, or the two levels, of exponent x and their blend.  An x
// that is not a number (the device form does not look) blends the last two levels into NaN and reads nothing outside the chain.
MCPT_HD void reflection_lookup(const mcpt_reflection_chain& c, const double* p, const double* d, double x, double* out)
{
    const int n = c.num_levels;
    int first[kReflectionMaxLevels];
    for (int l = 0, at = 0; l < n; l++) { first[l] = at; at += c.level_res[l] * c.level_res[l]; }
    if (n == 1 || x >= double(c.level_ns[0])) { reflection_level(p, c.level_res[0], d, out); return; }
    if (x <= double(c.level_ns[n - 1])) { reflection_level(p + size_t(first[n - 1]) * 3, c.level_res[n - 1], d, out); return; }
    int l = n - 2;
    for (int m = 0; m < n - 1; m++)
        if (x > double(c.level_ns[m + 1])) { l = m; break; }
    const double w0 = reflection_wt(double(c.level_ns[l])), w1 = reflection_wt(double(c.level_ns[l + 1]));
    const double a = (reflection_wt(x) - w0) / (w1 - w0);
    double v0[3], v1[3];
    reflection_level(p + size_t(first[l]) * 3, c.level_res[l], d, v0);
    if (a == 0.0) { for (int ch = 0; ch < 3; ch++) out[ch] = v0[ch]; return; }
    reflection_level(p + size_t(first[l + 1]) * 3, c.level_res[l + 1], d, v1);
    for (int ch = 0; ch < 3; ch++) out[ch] = (1.0 - a) * v0[ch] + a * v1[ch];
}

// What a bake's kernels share: the probes of the call and the workspace a chunk's rays and answers live in.  Entry e = (i * R * R + b)
// * S + j is sample j of texel b of probe i; a chunk holds the entries of texels first_texel .. first_texel + texels - 1 (numbered
// through the probes, i * R * R + b), entry first_texel * S + g at slot g.
struct ReflChunk {
    const double* p3;           // [n][3] all the call's probes
    const int32_t* id_base;     // [n] or null: i * R * R * S
    int R, S, sample_base;
    unsigned long long seed;
    long long first_texel, texels;
    double* rays6;              // [texels * S][6]
    int32_t* ids;               // [texels * S]
    const double* mean3;        // [texels * S][3] the query's answers, one sample each
    const int32_t* hits;        // [texels * S]
};

// rays6[g], ids[g] of the chunk's entries (entries == null, m = the chunk's rays), or of the listed entries entries[0 .. m) of the call
void launch_reflection_rays(const ReflChunk& c, const long long* d_entries, long long m, hipStream_t st);
// the fold of the chunk's answers, one lane per texel in j order, into radiance [n][R * R][3] and (each may be null) stderr, hits
void launch_reflection_fold(const ReflChunk& c, double* d_radiance, double* d_stderr, int32_t* d_hits, hipStream_t st);
// chain [n][T][3] from radiance [n][R * R][3]: one lane per output texel, the source staged through LDS (reflection.hip)
void launch_reflection_prefilter(const mcpt_reflection_chain& c, const double* d_radiance, int64_t n, double* d_chain, hipStream_t st);
// out3[q] of receivers q = 0 .. m - 1 (m >= 1): probe[q] outside 0 .. n - 1 gives +0.0
void launch_reflection_lookup(const mcpt_reflection_chain& c, const double* d_chain, int64_t n, const int32_t* d_probe, const double* d_d3, const double* d_x,
                              int64_t m, double* d_out3, hipStream_t st);

}  // namespace mcpt
