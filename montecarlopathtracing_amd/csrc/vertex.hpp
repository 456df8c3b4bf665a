// The three pieces of shade() a path vertex is made of (MTPC/pathTracing.cpp:137-266): what the surface looks like at the hit, one
// light sample, and Russian roulette + nextRay -- and the few expressions that join them into a path.  The megakernel (shade_path.hpp),
// the logic and finishing kernels (wavefront_logic.hip) and the pool engine's path mode (trace_pool.hpp) all shade with these, each in
// its own order and with its own way of tracing the rays.  One copy remains: shade_path's loop over every light spells light_sample out
// (it says why); tests hold the two equal bit for bit.
#pragma once
#include "dev_common.hpp"
#include "shade_common.hpp"
#include "light_tree.hpp"
#include "wavefront.hpp"

namespace mcpt {

// ---- what joins the pieces
// the throughput after a bounce of weight wgt that survived Russian roulette: T * wgt / P_RR
__device__ __forceinline__ V3 after_bounce(const V3& T, const V3& wgt)
{
    return mk(T.x * wgt.x * MCPT_INV_P_RR, T.y * wgt.y * MCPT_INV_P_RR, T.z * wgt.z * MCPT_INV_P_RR);
}
// The throughput after the bounce of a pixel's primary hit -- the first vertex of the per-pixel route, shaded by k_wf_logic<true> with
// T = 1 -- for a sample whose bounce ray there has type bt: after_bounce((1, 1, 1), wgt) with bounce_sample's wgt (kd / ks / 1: the pixel's
// kd from its PrimarySurface, its material's ks).  The same expression on the same operands as when the vertex was shaded, hence the same
// bits; with one light the first pass therefore does not store T, and whoever reads the T of such a vertex (the depth-1 logic pass, the
// finishing kernels when they adopt at depth 0) calls this instead.
__device__ __forceinline__ V3 first_vertex_throughput(const DScene& S, const WfArgs& a, int id, int bt)
{
    const PrimarySurface* ps = a.surf + a.hits[a.first_slot + id / a.spp].surf;
    const int type = bt & 7;
    const V3 wgt = type == RT_DIFFUSE ? ld3(ps->kd) : (type == RT_SPECULAR ? ld3(S.materials[ps->material].ks) : mk(1, 1, 1));
    return after_bounce(mk(1, 1, 1), wgt);
}
// L_dir += visibility * c as the reference forms it: a hidden light adds c * 0.0 (a zero of c's sign, NaN for an infinite c), not nothing
__device__ __forceinline__ void add_if_visible(V3& L_dir, const V3& c, bool vis)
{
    L_dir.x += vis ? c.x : c.x * 0.0;
    L_dir.y += vis ? c.y : c.y * 0.0;
    L_dir.z += vis ? c.z : c.z * 0.0;
}
// What a vertex's light samples are counted in, from nl = the shadow rays (planes) of a vertex: nplanes of them are the lights' -- ENV: an
// active environment has the last plane, PICK (1: MCPT_LIGHTS_ONE, 2: MCPT_LIGHTS_TREE): the lights share one plane, for the picked light;
// nlights = the Philox block base (dev_common.hpp), the scene's lights whatever nl says; folded: with one plane T * c and T * w / P_RR are
// formed when the vertex is shaded instead of when it is resolved (k_wf_logic).
struct PathLights { int nplanes, nlights; bool folded; };
template <bool ENV, int PICK>
__device__ __forceinline__ PathLights path_lights(const DScene& S, int nl)
{
    const int nplanes = ENV ? nl - 1 : nl;
    return {nplanes, PICK ? S.num_lights : nplanes, nl == 1};
}
// The RNG key of chunk-local sample id of a wavefront pass (WfState::id): its camera sample from the pass's base, its pixel through
// the slot list -- or given, where the caller has it at hand (the first logic pass: the pixel's record).
__device__ __forceinline__ RngKey sample_key(const WfArgs& a, int id, int pixel)
{
    RngKey key;
    key.k0 = (uint32_t)a.seed; key.k1 = (uint32_t)(a.seed >> 32);
    key.pixel = (uint32_t)pixel;
    key.sample = (uint32_t)(a.sample_base + id % a.spp);
    return key;
}
__device__ __forceinline__ RngKey sample_key(const WfArgs& a, int id)
{
    const int slot = a.first_slot + id / a.spp;
    return sample_key(a, id, a.pixels ? a.pixels[slot] : slot);
}

// interpolated normal and diffuse colour at p on leaf `leaf` (:147-160, texture lookup Q9 / D7)
__device__ __forceinline__ void vertex_surface(const DScene& S, int leaf, const V3& p, const DMaterial* m, V3& pn, V3& kd)
{
    const DTri* tr = S.tris + leaf;
    const DTriShade* sh = S.shade + leaf;
    const V3 g = barycentric_s(ld3(tr->v1), ld3(tr->v2), ld3(tr->v3), p);
    pn = (ld3(sh->vn1) * g.x + ld3(sh->vn2) * g.y) + ld3(sh->vn3) * g.z;
    if (m->has_map) {
        const double row = sh->vt1[0] * g.x + sh->vt2[0] * g.y + sh->vt3[0] * g.z;
        const double col = sh->vt1[1] * g.x + sh->vt2[1] * g.y + sh->vt3[1] * g.z;
        const double irow = row - floor(row), icol = col - floor(col);
        int rr = (int)(irow * m->map_h), cc = (int)(icol * m->map_w);
        rr = rr < 0 ? 0 : (rr > m->map_h - 1 ? m->map_h - 1 : rr);
        cc = cc < 0 ? 0 : (cc > m->map_w - 1 ? m->map_w - 1 : cc);
        const uint8_t* px = S.texels + m->tex_offset + ((size_t)rr * m->map_w + cc) * 3;
        kd = mk((double)px[2] * MCPT_INV_255, (double)px[1] * MCPT_INV_255, (double)px[0] * MCPT_INV_255);
    } else kd = ld3(m->kd);
}

// Light l seen from the vertex (:166-232).  Returns the material the shadow ray must reach for the light to count, or -2 when
// the light is behind the surface (the only case in which the shadow ray's answer is not used); direction = the shadow ray's
// direction (origin p + 0.01 direction), c = the contribution if visible.  sample_mat carries over from light to light as in
// the reference (a light whose area sample fails keeps the previous light's material).
__device__ __forceinline__ int light_sample(const DScene& S, const RngKey& key, uint32_t depth, int l, const V3& p, const V3& pn, const V3& kd,
                                            int& sample_mat, V3& direction, V3& c)
{
    const DLight* lt = S.lights + l;
    V3 xl = mk(0, 0, 0), vn = mk(0, 0, 0);
    double u0, u1, u2, u3;
    uniform4(key, depth, (uint32_t)l, u0, u1, u2, u3);
    const double rnd = u0 * S.area0;                                            // frozen static u1 range (Q1)
    const int jt = pick_light_triangle(S.light_cdf + lt->first, lt->ntri, lt->cdf_sorted != 0, rnd);
    if (jt >= 0) {
        const DLightTri* q = S.light_tris + lt->first + jt;
        sample_mat = lt->material;
        const double isum = frcp(u1 + u2 + u3);
        const double p1 = u1 * isum, p2 = u2 * isum, p3 = u3 * isum;
        xl = (ld3(q->v1) * p1 + ld3(q->v2) * p2) + ld3(q->v3) * p3;
        vn = (ld3(q->vn1) * p1 + ld3(q->vn2) * p2) + ld3(q->vn3) * p3;
    }
    direction = normalized_s(xl - p);
    const double kd_dots = dot(direction, pn);
    if (!(kd_dots > 0)) return -2;
    // (the reference also divides by |direction|, a unit vector: 1 to within the two ulps this arithmetic is held to)
    const double cos_theta = fabs(dot(direction, vn) * frcp(norm_s(vn)));
    const double cos_theta_hat = fabs(kd_dots * frcp(norm_s(pn)));
    const double dd = norm_s(xl - p);
    const double dist = (1.0 < dd) ? dd : 1.0;                                  // std::max(1.0, distance)
    const V3 intensity = ((ld3(lt->radiance) * cos_theta) * cos_theta_hat) * (frcp(sqr(dist)) * lt->total_area);
    c = mk(kd.x * intensity.x * kd_dots * MCPT_INV_PI, kd.y * intensity.y * kd_dots * MCPT_INV_PI, kd.z * intensity.z * kd_dots * MCPT_INV_PI);
    return sample_mat;
}

// MCPT_LIGHTS_ONE: the light picked at vertex `depth` of a camera sample, from slot 0 of Philox block nl + 3 (nl = the scene's lights; the
// lights' draws use blocks 0 .. nl-1, the bounce nl and nl + 1, the environment nl + 2).  The smallest l with u * Z < cdf[l], by binary
// search over 0 .. last: a light of weight 0 (cdf[l] == cdf[l-1]) is never picked.  inv_p = 1 / p_l, the host's quotient.
__device__ __forceinline__ int light_pick(const DLightPick& P, const RngKey& key, uint32_t depth, uint32_t nl, double& inv_p)
{
    const double x = uniform1(key, depth, nl + 3u) * P.Z;
    int lo = 0, hi = P.last;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (x < P.cdf[mid]) hi = mid; else lo = mid + 1; }
    inv_p = P.inv_pdf[lo];
    return lo;
}

// MCPT_LIGHTS_TREE: the light picked at the vertex (p, pn) at `depth` of a camera sample, and the probability it was picked with.  The draw is
// light_pick's (slot 0 of Philox block nl + 3), so every other draw keeps its value.  From the root, at every inner node the left child is
// taken with probability pL (light_tree.hpp: importance by distance and horizon) and the draw is stretched over the side taken; the tree is
// a median split, ceil(log2 nl) levels deep, and the descent keeps no stack.  pL is 1.0 (or 0.0) exactly where a side is culled or has
// weight 0: u / 1.0, pdf * 1.0 and (u - 0.0) / (1.0 - 0.0) change no bit, so those cases need no code of their own.
__device__ __forceinline__ int light_pick_at(const DLightPick& P, const RngKey& key, uint32_t depth, uint32_t nl, const V3& p, const V3& pn, double& pdf)
{
    double u = uniform1(key, depth, nl + 3u);
    pdf = 1.0;
    int n = 0, l;
    while ((l = P.nodes[n].left) >= 0) {
        const int r = P.nodes[n].right;
        const double pL = light_tree_left(P.nodes[l], P.nodes[r], p.x, p.y, p.z, pn.x, pn.y, pn.z);
        if (pL >= 1.0) n = l;
        else if (u < pL) { n = l; u = u / pL; pdf *= pL; }
        else { n = r; u = (u - pL) / (1.0 - pL); pdf *= (1.0 - pL); }
    }
    return ~l;
}

// MCPT_LIGHTS_ONE (PICK 1) and MCPT_LIGHTS_TREE (PICK 2): the one light sample of the vertex -- light_sample of the picked light (its own
// Philox block, no light before it to inherit a material from), c scaled by 1 / p_l.  Returns as light_sample does.
template <int PICK>
__device__ __forceinline__ int light_sample_one(const DScene& S, const RngKey& key, uint32_t depth, const V3& p, const V3& pn, const V3& kd, V3& direction, V3& c)
{
    double inv_p;
    int l;
    if constexpr (PICK == 2) {
        double pdf;
        l = light_pick_at(S.pick, key, depth, (uint32_t)S.num_lights, p, pn, pdf);
        inv_p = 1.0 / pdf;
    } else l = light_pick(S.pick, key, depth, (uint32_t)S.num_lights, inv_p);
    int sample_mat = -1;
    const int expect = light_sample(S, key, depth, l, p, pn, kd, sample_mat, direction, c);
    if (expect != -2) c = mk(c.x * inv_p, c.y * inv_p, c.z * inv_p);
    return expect;
}

#define MCPT_BT_NO_OFFSET 8         /* flag in a bounce type: the ray starts at the vertex itself (refraction, total reflection) */

// Russian roulette and nextRay (:3-11, :66-134, :234-263) at a vertex reached along -dir.  Returns -1 when the path ends here,
// else the ray type (| MCPT_BT_NO_OFFSET), with nd = direction of the bounce ray and wgt = kd / ks / 1.
__device__ __forceinline__ int bounce_sample(const RngKey& key, uint32_t depth, int nl, const DMaterial* m, const V3& dir, const V3& pn, const V3& kd,
                                             V3& nd, V3& wgt)
{
    if (depth + 1 >= MCPT_MAX_DEPTH_DEV) return -1;                            // D6
    double u_rr, u_fresnel, u_lobe, u_phi;
    uniform4(key, depth, (uint32_t)nl, u_rr, u_fresnel, u_lobe, u_phi);
    if (!(u_rr < MCPT_P_RR)) return -1;
    int btype = -1, at_vertex = 0;
    const V3 ks = ld3(m->ks);
    if (m->Ni > 1) {
        double n1, n2;
        const double cos_in = dot(neg(dir), pn);
        V3 normal;
        if (cos_in > 0) { normal = neg(pn); n1 = m->Ni; n2 = 1.0; }
        else { normal = pn; n1 = 1.0; n2 = m->Ni; }
        const double rf0 = sqr((n1 - n2) / (n1 + n2));
        const double fresnel = rf0 + (1.0f - rf0) * pow5(1.0f - fabs(cos_in));
        if (fresnel < u_fresnel) {
            V3 direction;
            at_vertex = MCPT_BT_NO_OFFSET;
            if (refract_dir(neg(dir), normal, n1 / n2, direction)) { nd = direction; btype = RT_TRANSMISSION; }
            else {
                const V3 incoming = neg(dir);
                nd = incoming - (normal * dot(incoming, normal)) * 2; btype = RT_SPECULAR;
            }
        }
    }
    if (btype < 0) {
        const double u_theta = uniform1(key, depth, (uint32_t)nl + 1u);
        const double ks_norm = norm_s(ks);
        if (ks_norm != 0 && norm_s(kd) * frcp(ks_norm) < u_lobe) {
            const V3 incoming = neg(dir);
            const V3 reflect = incoming - (pn * dot(incoming, pn)) * 2;
            nd = brdf_sample(u_phi, u_theta, reflect, RT_SPECULAR, m->Ns);
            btype = RT_SPECULAR;
        } else {
            nd = brdf_sample(u_phi, u_theta, pn, RT_DIFFUSE, m->Ns);
            btype = RT_DIFFUSE;
        }
    }
    wgt = btype == RT_DIFFUSE ? kd : (btype == RT_SPECULAR ? ks : mk(1, 1, 1));
    return btype | at_vertex;
}

}  // namespace mcpt
