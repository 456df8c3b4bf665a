// shade() as a loop over the path's vertices, one lane per path (the megakernel pipeline).
#pragma once
#include "dev_common.hpp"
#include "shade_common.hpp"
#include "kernels.hpp"
#include "env.hpp"
#include "vertex.hpp"

namespace mcpt {

// shade() (pathTracing.cpp:137-266) of a fresh camera sample that arrived along view_dir at `hit`, with the recursion unrolled into a
// loop: the recursion is a chain (one bounce per vertex), so L = sum_d T_d * Ldir_d with T_{d+1} = T_d * w_d / 0.6.  Every vertex is
// made of vertex.hpp's pieces, as in the wavefront kernels (but for the loop over every light, see there); every ray goes through the
// reference-shaped trace_closest.  ENV: S.env is
// active (env.hpp) -- one more shadow ray per vertex after the lights', and a SPECULAR / TRANSMISSION bounce ray that leaves the scene
// adds T' * Le.  PICK: the pick mode (1: MCPT_LIGHTS_ONE, 2: MCPT_LIGHTS_TREE) -- one shadow ray, for the light light_sample_one draws,
// instead of one per light; a light behind the surface is counted as skipped and not traced.  Without a pick (0) every light's shadow
// ray is traced and counted as the reference does, also where the light is behind the surface and the answer is not used.
template <bool ENV = false, int PICK = 0>
__device__ void shade_path(const DScene& S, const RngKey& key, V3 view_dir, Hit hit, double out[3], LaneStats& ls)
{
    const int nl = S.num_lights;
    Work w = {0, 0};
    V3 T = mk(1, 1, 1), L = mk(0, 0, 0), dir = neg(view_dir);
    int in_type = RT_TRANSMISSION;
    // the shadow ray towards `direction`: the material it reaches, -1 when it leaves the scene
    auto shadow = [&](const V3& direction) -> int {
        Ray rl; rl.o = hit.p + direction * 0.01; rl.d = direction;
        Hit inter;
        ls.shadow++;
        return trace_closest(S, rl, inter, w) ? S.tris[inter.leaf].material : -1;
    };
    for (uint32_t depth = 0;; depth++) {
        ls.shades++;
        if (depth > ls.depth) ls.depth = depth;
        const DMaterial* m = S.materials + S.tris[hit.leaf].material;
        if (m->light >= 0) {                                                    // :141-144
            const V3 rad = ld3(S.lights[m->light].radiance);
            if (depth == 0) L = rad;
            else if (in_type != RT_DIFFUSE) L = L + mul(T, rad);                // :247-261
            break;
        }
        V3 pn, kd;
        vertex_surface(S, hit.leaf, hit.p, m, pn, kd);

        // direct illumination, :166-232.  (The reference multiplies a light's intensity by its visibility, 1 or 0, before the product
        // with kd, as the loop over every light below does; add_if_visible adds c or c * 0.0.  The same bits: * 1.0 is exact and a
        // zero keeps its sign through positive factors -- the wavefront kernels form every light this way.)
        V3 L_dir = mk(0, 0, 0), direction, c;
        if constexpr (PICK) {
            const int expect = light_sample_one<PICK>(S, key, depth, hit.p, pn, kd, direction, c);
            if (expect != -2) add_if_visible(L_dir, c, shadow(direction) == expect);
            else ls.skipped++;
        } else {
            // light_sample() spelled out, the trace between the light point and the cosines as in the reference.  Written with
            // light_sample (c formed before the trace, add_if_visible after it) this loop gives the same bits and counters, but the
            // frame was slower: cornell-box 1280x720 SPP 256 on one MI355X, nine frames each, 4554.7 .. 4567.3 ms (median 4564.5) against
            // 4486.3 .. 4507.8 ms (median 4493.3) for this form -- 71 ms where the frames of one build spread over 21.5 ms.
            int sample_mat = -1;
            for (int l = 0; l < nl; l++) {
                const DLight* lt = S.lights + l;
                V3 xl = mk(0, 0, 0), vn = mk(0, 0, 0);
                double u0, u1, u2, u3;
                uniform4(key, depth, (uint32_t)l, u0, u1, u2, u3);
                const double rnd = u0 * S.area0;                                // frozen static u1 range (Q1)
                const int j = pick_light_triangle(S.light_cdf + lt->first, lt->ntri, lt->cdf_sorted != 0, rnd);
                if (j >= 0) {
                    const DLightTri* q = S.light_tris + lt->first + j;
                    sample_mat = lt->material;
                    const double isum = frcp(u1 + u2 + u3);
                    const double p1 = u1 * isum, p2 = u2 * isum, p3 = u3 * isum;
                    xl = (ld3(q->v1) * p1 + ld3(q->v2) * p2) + ld3(q->v3) * p3;
                    vn = (ld3(q->vn1) * p1 + ld3(q->vn2) * p2) + ld3(q->vn3) * p3;
                }
                direction = normalized_s(xl - hit.p);
                const double visibility = shadow(direction) == sample_mat ? 1 : 0;     // :213 (traced whether or not the light is in front)
                const double kd_dots = dot(direction, pn);
                if (kd_dots > 0) {
                    const double cos_theta = fabs(dot(direction, vn) * frcp(norm_s(vn)));
                    const double cos_theta_hat = fabs(kd_dots * frcp(norm_s(pn)));
                    const double dd = norm_s(xl - hit.p);
                    const double dist = (1.0 < dd) ? dd : 1.0;                  // std::max(1.0, distance)
                    const V3 intensity = (((ld3(lt->radiance) * cos_theta) * cos_theta_hat) * (frcp(sqr(dist)) * lt->total_area)) * visibility;
                    L_dir.x += kd.x * intensity.x * kd_dots * MCPT_INV_PI;
                    L_dir.y += kd.y * intensity.y * kd_dots * MCPT_INV_PI;
                    L_dir.z += kd.z * intensity.z * kd_dots * MCPT_INV_PI;
                }
            }
        }
        if constexpr (ENV) {                                                    // the environment: Philox block nl + 2, the ray must leave
            if (env_light_sample(S.env, key, depth, (uint32_t)nl, pn, kd, direction, c) != -2) add_if_visible(L_dir, c, shadow(direction) == -1);
        }
        L = L + mul(T, L_dir);

        // indirect illumination, :234-263
        Ray nr;
        V3 wgt;
        const int bt = bounce_sample(key, depth, nl, m, dir, pn, kd, nr.d, wgt);
        if (bt < 0) break;
        nr.o = (bt & MCPT_BT_NO_OFFSET) ? hit.p : hit.p + nr.d * 0.01;
        ls.bounce++;
        T = after_bounce(T, wgt);
        Hit next;
        if (!trace_closest(S, nr, next, w)) {
            if constexpr (ENV) L = env_escape(S.env, L, T, bt & 7, nr.d);
            break;
        }
        hit = next; dir = neg(nr.d); in_type = bt & 7;
    }
    ls.nodes += w.nodes; ls.tris += w.tris;
    out[0] = L.x; out[1] = L.y; out[2] = L.z;
}

// a camera ray that left the scene: Le of its direction, unweighted (as an emitter at depth 0)
__device__ __forceinline__ void env_camera_miss(const DScene& S, const V3& d, double out[3])
{
    const V3 le = env_eval(S.env, d);
    out[0] = le.x; out[1] = le.y; out[2] = le.z;
}

}  // namespace mcpt
