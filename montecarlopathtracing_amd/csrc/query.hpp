// Radiance queries (mcpt_query_radiance, mcpt.h): the path tracer behind a caller's ray list instead of the scene's camera.  A query is a
// camera sample of the per-sample route whose ray the caller gives -- or, MCPT_QUERY_HEMISPHERE, draws cosine-weighted about a normal, or,
// a light probe (mcpt_query_sh), uniformly over the sphere -- and whose RNG key is (seed, id, k).  query_ray is the one device function every consumer calls (k_query_pass, k_query_samples,
// k_query_rays), the counterpart of camera_ray (camera.hpp).  fp64 without contraction (-ffp-contract=off), in the operation order mcpt.h
// states.
#pragma once
#include <hip/hip_runtime.h>

#include "camera.hpp"
#include "dev_common.hpp"
#include "device_scene.hpp"

namespace mcpt {

#define MCPT_QUERY_KIND_RAY        0     /* == MCPT_QUERY_RAY */
#define MCPT_QUERY_KIND_HEMISPHERE 1     /* == MCPT_QUERY_HEMISPHERE */
// Internal: a light probe (mcpt_query_sh), a direction uniform over the sphere from the position itself.  No public entry that takes a
// kind accepts it; its list holds 3 doubles per entry, not 6.  A probe is meant to sit in free space: its rays leave the point with no
// offset (the ray kind's convention), so a caller who puts one on a surface lifts it off first.  MCPT_QUERY_KIND_SPHERE = 2 is defined
// beside DQuery (device_scene.hpp), where the host code sees it as well.

// doubles per list entry
__device__ __host__ __forceinline__ int query_stride(int kind) { return kind == MCPT_QUERY_KIND_SPHERE ? 3 : 6; }

// the ray of sample k of the query q[0..6) (a probe: q[0..3)) with id `id`
__device__ __forceinline__ void query_ray(int kind, const double* __restrict__ q, unsigned long long seed, int id, int k, V3& o, V3& d)
{
    if (kind == MCPT_QUERY_KIND_SPHERE) {
        RngKey key; key.k0 = (uint32_t)seed; key.k1 = (uint32_t)(seed >> 32); key.pixel = (uint32_t)id; key.sample = (uint32_t)k;
        double u0, u1, u2, u3;
        uniform4(key, MCPT_LENS_RNG_DEPTH, 0u, u0, u1, u2, u3);
        const double z = 1.0 - 2.0 * u0, w = 1.0 - z * z, r = sqrt(w > 0.0 ? w : 0.0), phi = 6.283185307179586 * u1;
        double sn, co;
        sincos(phi, &sn, &co);
        d = normalized(mk(r * co, r * sn, z));
        o = ld3(q);
        return;
    }
    const V3 a = ld3(q), b = ld3(q + 3);
    if (kind == MCPT_QUERY_KIND_RAY) { o = a; d = b; return; }
    const V3 n = normalized(b);
    const double ax = fabs(n.x), ay = fabs(n.y), az = fabs(n.z);
    // the coordinate axis on which |n^| is smallest, the lowest among equals
    const V3 e = (ax <= ay && ax <= az) ? mk(1.0, 0.0, 0.0) : (ay <= az ? mk(0.0, 1.0, 0.0) : mk(0.0, 0.0, 1.0));
    const V3 t = normalized(cross(e, n));
    const V3 s = cross(n, t);
    RngKey key; key.k0 = (uint32_t)seed; key.k1 = (uint32_t)(seed >> 32); key.pixel = (uint32_t)id; key.sample = (uint32_t)k;
    double u0, u1, u2, u3;
    uniform4(key, MCPT_LENS_RNG_DEPTH, 0u, u0, u1, u2, u3);
    const double r = sqrt(u0), phi = 6.283185307179586 * u1;
    const double w = 1.0 - u0, z = sqrt(w > 0.0 ? w : 0.0);
    double sn, co;
    sincos(phi, &sn, &co);
    d = normalized((t * (r * co) + s * (r * sn)) + n * z);
    o = a + d * 0.01;
}

}  // namespace mcpt
