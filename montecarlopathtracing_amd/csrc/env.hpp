// The environment light (mcpt_device_set_environment, mcpt.h): radiance of a ray that leaves the scene, and one importance-sampled shadow
// ray per vertex.  The one pair of device functions every consumer calls -- the megakernel (shade_path.hpp), the logic and finishing
// kernels (wavefront_logic.hip, trace_pool.hpp), the folds, and the mcpt_environment_* seams.  fp64 without contraction
// (-ffp-contract=off), in the operation order mcpt.h states; the tables are built on the host (environment.cpp).
#pragma once
#include "dev_common.hpp"
#include "shade_common.hpp"

namespace mcpt {

#define MCPT_ENV_PI 3.141592653589793
#define MCPT_ENV_TWO_PI 6.283185307179586

// texel (i, j) of the map and its radiance, scale * texel
__device__ __forceinline__ V3 env_texel(const DEnv& E, int i, int j)
{
    const float* t = E.rgb + ((size_t)i * E.W + j) * 3;
    return mk(E.scale * (double)t[0], E.scale * (double)t[1], E.scale * (double)t[2]);
}

// Le(d): nearest texel of direction d (need not be normalised in y: d.y is clamped to [-1, 1])
__device__ __forceinline__ V3 env_eval(const DEnv& E, const V3& d)
{
    double phi = atan2(d.z, d.x);
    if (phi < 0.0) phi += MCPT_ENV_TWO_PI;
    int j = (int)floor(phi * (double)E.W / MCPT_ENV_TWO_PI);
    j = j < E.W - 1 ? j : E.W - 1;
    j = j > 0 ? j : 0;
    const double y = fmin(fmax(d.y, -1.0), 1.0);
    int lo = 0, hi = E.H - 1;                                       // the row with c[i+1] < y <= c[i] (the last row takes y = -1)
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (E.c[mid + 1] < y) hi = mid; else lo = mid + 1; }
    return env_texel(E, lo, j);
}

// first k with rnd < cdf[k], clamped to n - 1 (pick_light_triangle's search; rnd < cdf[n-1] whenever u < 1)
__device__ __forceinline__ int env_pick(const double* __restrict__ cdf, int n, double rnd)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (rnd < cdf[mid]) hi = mid; else lo = mid + 1; }
    return lo < n ? lo : n - 1;
}

// A direction drawn in proportion to luminance x solid angle from uniforms u0..u3: texel (i, j), direction d, pdf = lum_ij / Z (solid
// angle) and the texel's radiance.
__device__ __forceinline__ void env_sample_u(const DEnv& E, double u0, double u1, double u2, double u3, V3& d, double& pdf, V3& le)
{
    const int i = env_pick(E.marg, E.H, u0 * E.Z);
    const double* row = E.cond + (size_t)i * E.W;
    const int j = env_pick(row, E.W, u1 * row[E.W - 1]);
    const double ct = E.c[i] + (E.c[i + 1] - E.c[i]) * u2;
    const double st = sqrt(fmax(0.0, 1.0 - ct * ct));
    const double phi = (MCPT_ENV_TWO_PI * ((double)j + u3)) / (double)E.W;
    double sp, cp;
    sincos(phi, &sp, &cp);
    d = mk(st * cp, ct, st * sp);
    const float* t = E.rgb + ((size_t)i * E.W + j) * 3;
    const double lum = (0.2126 * (double)t[0] + 0.7152 * (double)t[1]) + 0.0722 * (double)t[2];
    pdf = lum / E.Z;
    le = env_texel(E, i, j);
}

// the environment's draw at vertex `depth` of a camera sample: Philox block nl + 2 (nl = the scene's lights)
__device__ __forceinline__ void env_sample(const DEnv& E, const RngKey& key, uint32_t depth, uint32_t nl, V3& d, double& pdf, V3& le)
{
    double u0, u1, u2, u3;
    uniform4(key, depth, nl + 2u, u0, u1, u2, u3);
    env_sample_u(E, u0, u1, u2, u3, d, pdf, le);
}

// The environment's light sample at vertex p with normal pn and diffuse colour kd: -2 when the direction is below the surface (no
// shadow ray), else -1 -- the shadow ray (origin p + 0.01 direction) must leave the scene -- with c = the contribution if it does:
// c = kd * Le * (((k / |pn|) / pi) / pdf), k = direction . pn.
__device__ __forceinline__ int env_light_sample(const DEnv& E, const RngKey& key, uint32_t depth, uint32_t nl, const V3& pn, const V3& kd,
                                                V3& direction, V3& c)
{
    double pdf;
    V3 le;
    env_sample(E, key, depth, nl, direction, pdf, le);
    const double k = dot(direction, pn);
    if (!(k > 0)) return -2;
    const double g = ((k / sqrt(dot(pn, pn))) / MCPT_ENV_PI) / pdf;
    c = mk((kd.x * le.x) * g, (kd.y * le.y) * g, (kd.z * le.z) * g);
    return -1;
}

// what a bounce ray of type `type` that left the scene along d adds to L: T' * Le(d) for SPECULAR and TRANSMISSION, T' = the throughput
// the next vertex would have had; nothing for DIFFUSE
__device__ __forceinline__ V3 env_escape(const DEnv& E, const V3& L, const V3& Tn, int type, const V3& d)
{
    if ((type & 7) == RT_DIFFUSE) return L;
    const V3 le = env_eval(E, d);
    return L + mul(Tn, le);
}

}  // namespace mcpt
