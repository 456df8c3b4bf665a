// The camera ray of one camera sample (pixel, k) under a lens (mcpt_device_set_lens, mcpt.h): the one device function every consumer
// calls -- the wavefront's per-sample route (k_camera_pass), the megakernel (k_shade_samples_lens), k_sample_radiance_lens and the
// mcpt_camera_rays seam.  fp64 without contraction (-ffp-contract=off), in the operation order mcpt.h states.
#pragma once
#include <hip/hip_runtime.h>

#include "dev_common.hpp"
#include "device_scene.hpp"

namespace mcpt {

#define MCPT_LENS_FLAG_JITTER     1      /* == MCPT_LENS_JITTER */
#define MCPT_LENS_FLAG_PER_SAMPLE 2      /* == MCPT_LENS_PER_SAMPLE */
#define MCPT_LENS_RNG_DEPTH 0xFFFFu      /* the Philox depth of the camera uniforms: no path vertex has it (MCPT_MAX_DEPTH = 64) */

__device__ __forceinline__ void camera_ray(const DLens& c, unsigned long long seed, int pixel, int k, V3& o, V3& d)
{
    const V3 eye = ld3(c.eye);
    V3 q = ld3(c.pos + (size_t)pixel * 3);
    const bool jitter = (c.flags & MCPT_LENS_FLAG_JITTER) != 0, thin = c.aperture > 0.0;
    double u0 = 0.0, u1 = 0.0, u2 = 0.0, u3 = 0.0;
    if (jitter || thin) {
        RngKey key; key.k0 = (uint32_t)seed; key.k1 = (uint32_t)(seed >> 32); key.pixel = (uint32_t)pixel; key.sample = (uint32_t)k;
        uniform4(key, MCPT_LENS_RNG_DEPTH, 0u, u0, u1, u2, u3);
    }
    if (jitter) q = (q + ld3(c.pdx) * u0) - ld3(c.pdy) * u1;        // a uniform point of the pixel square below-right of the corner
    if (!thin) {                                                     // pinhole: the reference's primary ray when q is the corner
        o = eye;
        d = normalized(q - eye);
        return;
    }
    const V3 f = eye + (q - eye) * c.focus_scale;                    // where the pinhole ray through q meets the plane in focus
    const double r = c.aperture * sqrt(u2), phi = 6.283185307179586 * u3;
    double s, co;
    sincos(phi, &s, &co);
    o = (eye + ld3(c.xhat) * (r * co)) + ld3(c.yhat) * (r * s);
    d = normalized(f - o);
}

}  // namespace mcpt
