// Direct light from a caller's own lights (mcpt.h: direct light): the one copy of the light arithmetic -- what a light is once its
// constants are formed (direct_prepare), the shadow ray and the geometric factor g of one slot (direct_slot), and the fold of an entry's
// slots into irradiance, error, per-light irradiance and visibility (DirectFold) --, compiled for the GPU (direct.hip: k_direct,
// k_direct_rays) and for the host (direct_api.cpp: the light table, mcpt_direct_fold_host; tests/direct_sanitize_main.cpp);
// tests/direct_ref.py restates it in numpy.  fp64, no contraction (-ffp-contract=off), IEEE division and sqrt, every expression in the
// order mcpt.h writes it; only + - * / and sqrt enter.  The launch interface of the kernels is at the end.  The walk that answers a
// shadow ray is any_hit_walk.hpp's: device code, which only direct.hip includes.
#pragma once
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mcpt.h"

#ifndef MCPT_HD
#if defined(__HIPCC__)
#define MCPT_HD __host__ __device__ __forceinline__
#else
#define MCPT_HD inline
#endif
#endif

namespace mcpt {

#define MCPT_DIRECT_RNG_DEPTH 0xFFFEu    /* the Philox depth of a rectangle's samples, beside MCPT_LENS_RNG_DEPTH: no path vertex, no camera draw */
constexpr int32_t kDirectMaxLights = 4096;              // the light index is the Philox block, a 16-bit field
constexpr int64_t kDirectSlotMax = 2147483647;          // n * R

// ---- a light as the kernels read it ------------------------------------------------------------------------------------------------
// The caller's record with its constants formed once, on the host, by the expressions mcpt.h writes: s = s^ (SPOT, DIRECTIONAL) or N^
// (RECT), A = |cross(u, v)| (RECT).  160 bytes; the table of a call lives in the device's own pinned and device copies.
struct DirectLight {
    int32_t type, flags;
    double p[3], u[3], v[3], color[3], s[3];
    double A, cos_inner, cos_outer, range;
};

MCPT_HD double direct_len(const double* a) { return sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); }

// Vertex::cross (dev_common.hpp: cross)
MCPT_HD void direct_cross(const double* a, const double* b, double* c)
{
    c[0] = a[1] * b[2] - b[1] * a[2];
    c[1] = b[0] * a[2] - a[0] * b[2];
    c[2] = a[0] * b[1] - b[0] * a[1];
}

// slots of one light: a delta light has one, a rectangle spp
MCPT_HD int32_t direct_light_slots(int32_t type, int32_t spp) { return type == MCPT_LIGHT_RECT ? spp : 1; }

MCPT_HD DirectLight direct_prepare(const mcpt_direct_light& L)
{
    DirectLight D;
    D.type = L.type; D.flags = L.flags;
    for (int c = 0; c < 3; c++) { D.p[c] = L.position[c]; D.u[c] = L.u[c]; D.v[c] = L.v[c]; D.color[c] = L.color[c]; D.s[c] = 0.0; }
    D.A = 0.0; D.cos_inner = L.cos_inner; D.cos_outer = L.cos_outer; D.range = L.range;
    if (L.type == MCPT_LIGHT_SPOT || L.type == MCPT_LIGHT_DIRECTIONAL) {
        const double l = direct_len(L.direction);
        D.s[0] = L.direction[0] / l; D.s[1] = L.direction[1] / l; D.s[2] = L.direction[2] / l;
    } else if (L.type == MCPT_LIGHT_RECT) {
        double N[3];
        direct_cross(L.u, L.v, N);
        D.A = direct_len(N);
        D.s[0] = N[0] / D.A; D.s[1] = N[1] / D.A; D.s[2] = N[2] / D.A;
    }
    return D;
}

// ---- one slot ----------------------------------------------------------------------------------------------------------------------
// The shadow ray and the factor g of one slot; a SKIPPED slot is o = a, d = 0, tmax = 0, g = +0.0, which is what the seam writes.  A slot
// is traced iff g > 0: the last skip of every light is "unless g > 0", so the fold can read it from g alone.
struct DirectSlot {
    double o[3], d[3], tmax, g;
};

MCPT_HD DirectSlot direct_skipped(const double* a)
{
    DirectSlot s;
    s.o[0] = a[0]; s.o[1] = a[1]; s.o[2] = a[2];
    s.d[0] = 0.0; s.d[1] = 0.0; s.d[2] = 0.0;
    s.tmax = 0.0; s.g = 0.0;
    return s;
}

MCPT_HD void direct_ray(const double* a, const double* w, double bias, DirectSlot& s)
{
    const double bx = w[0] * bias, by = w[1] * bias, bz = w[2] * bias;
    s.o[0] = a[0] + bx; s.o[1] = a[1] + by; s.o[2] = a[2] + bz;
    s.d[0] = w[0]; s.d[1] = w[1]; s.d[2] = w[2];
}

// a = the receiver's position, nh = its n^ (direct_normal), xi1, xi2 = the sample's uniforms (read by a rectangle only)
MCPT_HD DirectSlot direct_slot(const DirectLight& D, const double* a, const double* nh, double bias, double xi1, double xi2)
{
    DirectSlot s = direct_skipped(a);
    double w[3], g;
    if (D.type == MCPT_LIGHT_DIRECTIONAL) {
        w[0] = -D.s[0]; w[1] = -D.s[1]; w[2] = -D.s[2];
        const double cr = (nh[0] * w[0] + nh[1] * w[1]) + nh[2] * w[2];
        if (!(cr > 0.0)) return s;
        g = cr;
        if (!(g > 0.0)) return s;
        direct_ray(a, w, bias, s);
        s.tmax = INFINITY; s.g = g;
        return s;
    }
    double y[3] = {D.p[0], D.p[1], D.p[2]};
    if (D.type == MCPT_LIGHT_RECT)
        for (int c = 0; c < 3; c++) y[c] = (D.p[c] + D.u[c] * xi1) + D.v[c] * xi2;
    const double L[3] = {y[0] - a[0], y[1] - a[1], y[2] - a[2]};
    const double r2 = (L[0] * L[0] + L[1] * L[1]) + L[2] * L[2];
    if (!(r2 > 0.0 && r2 < INFINITY)) return s;
    const double r = sqrt(r2);
    w[0] = L[0] / r; w[1] = L[1] / r; w[2] = L[2] / r;
    const double cr = (nh[0] * w[0] + nh[1] * w[1]) + nh[2] * w[2];
    if (!(cr > 0.0)) return s;
    if (D.type == MCPT_LIGHT_RECT) {
        double cl = -((D.s[0] * w[0] + D.s[1] * w[1]) + D.s[2] * w[2]);
        if (D.flags & MCPT_LIGHT_TWO_SIDED) cl = fabs(cl);
        if (!(cl > 0.0)) return s;
        g = ((cr * cl) / r2) * D.A;
    } else {
        if (D.range > 0.0 && r > D.range) return s;
        g = cr / r2;
        if (D.type == MCPT_LIGHT_SPOT) {
            const double cs = -((D.s[0] * w[0] + D.s[1] * w[1]) + D.s[2] * w[2]);
            double x = (cs - D.cos_outer) / (D.cos_inner - D.cos_outer);
            if (!(x > 0.0)) return s;
            x = x < 1.0 ? x : 1.0;
            const double f = (x * x) * (3.0 - 2.0 * x);
            g = g * f;
        }
    }
    if (!(g > 0.0)) return s;
    direct_ray(a, w, bias, s);
    s.tmax = r - bias; s.g = g;
    return s;
}

// the hemisphere kind's n^ of an entry's normal b (query.hpp: normalized)
MCPT_HD void direct_normal(const double* b, double* nh)
{
    const double l = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    nh[0] = b[0] / l; nh[1] = b[1] / l; nh[2] = b[2] / l;
}

// ---- the fold of one entry ---------------------------------------------------------------------------------------------------------
// begin(); per light: light_begin(), add(light, g, occluded) for each of its slots in order, light_end(light, spp) -- after which El
// and vis are the light's --; E and V hold the entry's sums, stderr = sqrt(V).
struct DirectFold {
    double E[3], V[3], s1[3], s2[3], El[3], vis;
    int32_t traced, lit;

    MCPT_HD void begin() { for (int c = 0; c < 3; c++) { E[c] = 0.0; V[c] = 0.0; } }
    MCPT_HD void light_begin()
    {
        for (int c = 0; c < 3; c++) { s1[c] = 0.0; s2[c] = 0.0; El[c] = 0.0; }
        traced = 0; lit = 0;
    }
    MCPT_HD void add(const DirectLight& D, double g, bool occluded)
    {
        const bool tr = g > 0.0, open = tr && !occluded;
        traced += tr ? 1 : 0;
        lit += open ? 1 : 0;
        for (int c = 0; c < 3; c++) {
            const double x = open ? D.color[c] * g : 0.0;
            if (D.type == MCPT_LIGHT_RECT) { s1[c] += x; s2[c] += x * x; }
            else El[c] = x;
        }
    }
    MCPT_HD void light_end(const DirectLight& D, int32_t spp)
    {
        for (int c = 0; c < 3; c++) {
            double se2 = 0.0;
            if (D.type == MCPT_LIGHT_RECT) {
                El[c] = s1[c] / spp;
                if (spp >= 2) {
                    const double var = (s2[c] - s1[c] * s1[c] / spp) / (spp - 1);       // dev_common.hpp: progressive_se2
                    se2 = (var > 0.0 ? var : 0.0) / spp;
                }
            }
            E[c] += El[c];
            V[c] += se2;
        }
        vis = traced ? double(lit) / double(traced) : 0.0;
    }
};

// ---- launch interface (direct.hip) ------------------------------------------------------------------------------------------------
struct DScene;
struct DCounters;
// what both kernels read of a call: the entries (q6 [n][6], ids [n] or null), the light table (device memory, nl records) and the draw
struct DirectCall {
    const double* q6;
    const int32_t* ids;
    long long n;
    const DirectLight* lights;
    int32_t nl, spp, sample_base;
    unsigned long long seed;
    double bias;
};
// the query: irradiance3 [n][3] and (each may be null) stderr3 [n][3], per_light3 [n][nl][3], visibility [n][nl].  fast: any_lane_fast, else
// the definition.  n > 0.
void launch_direct(const DScene& S, bool fast, const DirectCall& c, double* d_irradiance3, double* d_stderr3, double* d_per_light3, double* d_visibility,
                   DCounters* ctr, int cus, hipStream_t st);
// the seam: rays6 [n * R][6], tmax [n * R], g [n * R], R slots per entry
void launch_direct_rays(const DirectCall& c, long long R, double* d_rays6, double* d_tmax, double* d_g, hipStream_t st);
// a map's scatter: the `width` doubles of list entry i to texel T = texels[i], as they are; a null d_out is skipped.  n_list * width
// <= 3 * (2^31 - 1).
void launch_direct_scatter(const int32_t* d_texels, long long n_list, int width, const double* d_in, double* d_out, hipStream_t st);

}  // namespace mcpt
