// The shading normal of a baked surface sample (mcpt.h: baked frames, "baked radiance"), the one copy of its rule: baked.hip's shading forms
// the normal for the diffuse lookup, baked_specular.hip's specular pass forms it again for the mirror direction.  Device only.
#pragma once
#include "baked.hpp"
#include "dev_common.hpp"

namespace mcpt {

// n = pn of mcpt_trace_closest goes in; it is replaced by the face's stored normal when it cannot be used, and turned towards the origin
// of the ray of direction d under MCPT_BAKED_FACE_VIEWER.  (baked.hip calls hit_normal itself, at the place it always has: with that call
// in here too its shading kernels come out with other register counts -- 86 / 136 / 190 for 98 / 122 / 190)
__device__ __forceinline__ void baked_normal_rule(const DTri* tr, const V3& d, int flags, double* n)
{
    if (baked_normal_bad(n))
        for (int c = 0; c < 3; c++) n[c] = tr->n[c];
    const double dd[3] = {d.x, d.y, d.z};
    if (flags & MCPT_BAKED_FACE_VIEWER) baked_face_viewer(dd, n);
}

// the normal at the hit (leaf lf, distance t, point p) of a ray of direction d: what baked_sample puts into q[3..5]
__device__ __forceinline__ void baked_normal(const DScene& S, const DTri* tr, int lf, double t, const V3& p, const V3& d, int flags, double* n)
{
    Hit h;
    h.leaf = lf; h.t = t; h.p = p;
    const V3 pn = hit_normal(S, h);
    n[0] = pn.x; n[1] = pn.y; n[2] = pn.z;
    baked_normal_rule(tr, d, flags, n);
}

}  // namespace mcpt
