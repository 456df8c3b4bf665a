// C ABI, baked specular (include/mcpt.h: mcpt_reflection_volume_lookup*, mcpt_baked_radiance_specular*, mcpt_render_baked_specular*):
// reflection probes on the probes of a volume grid, looked up by position, direction and exponent, and baked radiance and baked frames
// with ks * R added to their surface samples.  The baked calls are baked_api.cpp's own loops with the specular pass
// (baked_specular.hip) between a chunk's shading and its fold; the workspace, the gate, the lease, the staging and the chunk plan are
// theirs.  The lookup's arithmetic is reflection_volume.hpp's, compiled here for the host form.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>
#include <string>

#include "baked_specular.hpp"
#include "handles.hpp"

using namespace mcpt;

// what every call refuses of a reflection volume's grid, chain and visibility, without looking at the arrays
static int volume_check(const mcpt_volume_grid* g, const mcpt_reflection_chain* c, bool chain_data, const void* chain, const void* moments,
                        const mcpt_volume_visibility* v)
{
    if (const int rc = volume_grid_check(g)) return rc;
    if (const int rc = reflection_chain_check(c)) return rc;
    if (chain_data && !chain) return fail(MCPT_ERR_ARG, "null chain data");
    if (moments)
        if (const int rc = volume_visibility_check(v)) return rc;
    return MCPT_OK;
}

static int lookup_check(const mcpt_volume_grid* g, const mcpt_reflection_chain* c, const void* chain, const void* moments, const mcpt_volume_visibility* v,
                        const void* q6, const void* d3, const void* x, int64_t m, const void* out3)
{
    if (const int rc = volume_check(g, c, false, chain, moments, v)) return rc;
    if (const int rc = count_check(m, "receivers")) return rc;
    if (m > 0 && (!chain || !q6 || !d3 || !x || !out3)) return fail(MCPT_ERR_ARG, "null chain, receiver list, directions, exponents or radiance");
    return MCPT_OK;
}

// ... and what the host-pointer forms of the lookup refuse of the arrays themselves
static int lookup_arrays_check(const mcpt_volume_grid& g, const mcpt_reflection_chain& c, const double* chain, const double* q6, const double* d3,
                               const double* x, int64_t m)
{
    if (const int rc = reflection_finite_check(chain, size_t(volume_probes(g)) * size_t(reflection_chain_texels(c)) * 3, "the chain")) return rc;
    for (int64_t i = 0; i < m; i++) {
        const double* q = q6 + i * 6;
        for (int k = 0; k < 6; k++)
            if (!std::isfinite(q[k])) return fail(MCPT_ERR_ARG, "receiver " + std::to_string(i) + ": component that is not finite");
        const double nl = std::sqrt((q[3] * q[3] + q[4] * q[4]) + q[5] * q[5]);
        if (!(std::isfinite(nl) && nl > 0.0)) return fail(MCPT_ERR_ARG, "receiver " + std::to_string(i) + ": the normal must have a non-zero finite length");
        const double* d = d3 + i * 3;
        const double l = (std::fabs(d[0]) + std::fabs(d[1])) + std::fabs(d[2]);
        if (!(l > 0.0 && std::isfinite(l))) return fail(MCPT_ERR_ARG, "receiver " + std::to_string(i) + ": direction not finite, zero, or too long");
        if (!(std::isfinite(x[i]) && x[i] >= 0.0)) return fail(MCPT_ERR_ARG, "receiver " + std::to_string(i) + ": the exponent must be finite and >= 0");
    }
    return MCPT_OK;
}

// a checked volume as the kernels and the host form read it
static ReflVolume volume_of(const mcpt_volume_grid& g, const mcpt_reflection_chain& c, const double* chain, const uint8_t* valid, const double* moments,
                            const mcpt_volume_visibility* v)
{
    ReflVolume V{};
    V.grid = g;
    V.chain = c;
    V.texels = reflection_chain_texels(c);
    V.data = chain;
    V.valid = valid;
    if (moments) { V.visible = 1; V.vis = *v; V.moments = moments; }
    return V;
}

// the device copies of a host-pointer volume among the call's
static int volume_upload(const mcpt_volume_grid& g, const mcpt_reflection_chain& c, const double* chain, const uint8_t* valid, const double* moments,
                         const mcpt_volume_visibility* v, Staging& S, const double*& d_chain, const uint8_t*& d_valid, const double*& d_moments)
{
    const size_t probes = size_t(volume_probes(g));
    const size_t bins = moments ? size_t(v->res) * size_t(v->res) : 0;
    if (const int rc = S.in(chain, probes * size_t(reflection_chain_texels(c)) * 3, "the volume's chains", d_chain)) return rc;
    if (const int rc = S.in(valid, probes, "the volume's mask", d_valid)) return rc;
    if (const int rc = S.in(moments, probes * bins * 2, "the volume's moments", d_moments)) return rc;
    return MCPT_OK;
}

// what the baked calls refuse of their specular source, in the header's order
static int specular_check(const mcpt_baked_specular* sp)
{
    if (!sp) return fail(MCPT_ERR_ARG, "null baked specular source");
    if (sp->flags != 0) return fail(MCPT_ERR_ARG, "mcpt_baked_specular.flags must be 0");
    for (int i = 0; i < 4; i++)
        if (sp->reserved[i] != 0) return fail(MCPT_ERR_ARG, "mcpt_baked_specular.reserved must be 0");
    return volume_check(sp->grid, sp->chain, true, sp->chain_data, sp->moments, sp->visibility);
}

static int specular_outputs_check(const mcpt_baked_specular_outputs* so)
{
    if (so && (so->reserved[0] != 0 || so->reserved[1] != 0)) return fail(MCPT_ERR_ARG, "mcpt_baked_specular_outputs.reserved must be 0");
    return MCPT_OK;
}

static int radiance_check(const mcpt_baked_source* s, const mcpt_baked_specular* sp, const void* rays6, int64_t n, int32_t flags, const mcpt_baked_outputs* o,
                          const mcpt_baked_specular_outputs* so)
{
    if (const int rc = baked_source_check(s)) return rc;
    if (const int rc = specular_check(sp)) return rc;
    if (const int rc = baked_radiance_args_check(rays6, n, flags, o)) return rc;
    return specular_outputs_check(so);
}

static int frame_check(const mcpt_baked_source* s, const mcpt_baked_specular* sp, const mcpt_baked_frame_params* p, const void* img)
{
    if (const int rc = baked_source_check(s)) return rc;
    if (const int rc = specular_check(sp)) return rc;
    return baked_frame_args_check(p, img);
}

static ReflVolume volume_of(const mcpt_baked_specular& sp)
{
    return volume_of(*sp.grid, *sp.chain, sp.chain_data, sp.valid, sp.moments, sp.visibility);
}

extern "C" {

int mcpt_reflection_volume_lookup_host(const mcpt_volume_grid* g, const mcpt_reflection_chain* c, const double* chain, const uint8_t* valid,
                                       const double* moments, const mcpt_volume_visibility* v, const double* q6, const double* d3, const double* x,
                                       int64_t m, double* out3, int32_t* corners)
{
    if (const int rc = lookup_check(g, c, chain, moments, v, q6, d3, x, m, out3)) return rc;
    if (m == 0) return MCPT_OK;
    if (const int rc = lookup_arrays_check(*g, *c, chain, q6, d3, x, m)) return rc;
    const ReflVolume V = volume_of(*g, *c, chain, valid, moments, v);
    for (int64_t i = 0; i < m; i++) {
        const int n = V.visible ? reflection_volume_lookup<true>(V, q6 + i * 6, d3 + i * 3, x[i], out3 + i * 3)
                                : reflection_volume_lookup<false>(V, q6 + i * 6, d3 + i * 3, x[i], out3 + i * 3);
        if (corners) corners[i] = n;
    }
    return MCPT_OK;
}

int mcpt_reflection_volume_lookup_device(mcpt_device* d, const mcpt_volume_grid* g, const mcpt_reflection_chain* c, const double* d_chain,
                                         const uint8_t* d_valid, const double* d_moments, const mcpt_volume_visibility* v, const double* d_q6,
                                         const double* d_d3, const double* d_x, int64_t m, double* d_out3, int32_t* d_corners, void* stream)
{
    if (const int rc = lookup_check(g, c, d_chain, d_moments, v, d_q6, d_d3, d_x, m, d_out3)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (m == 0) return MCPT_OK;
    launch_reflection_volume_lookup(volume_of(*g, *c, d_chain, d_valid, d_moments, v), d_q6, d_d3, d_x, m, d_out3, d_corners, static_cast<hipStream_t>(stream));
    return launch_result();
}

int mcpt_reflection_volume_lookup(mcpt_device* d, const mcpt_volume_grid* g, const mcpt_reflection_chain* c, const double* chain, const uint8_t* valid,
                                  const double* moments, const mcpt_volume_visibility* v, const double* q6, const double* d3, const double* x, int64_t m,
                                  double* out3, int32_t* corners)
{
    if (const int rc = lookup_check(g, c, chain, moments, v, q6, d3, x, m, out3)) return rc;
    if (m > 0)
        if (const int rc = lookup_arrays_check(*g, *c, chain, q6, d3, x, m)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (m == 0) return MCPT_OK;
    const size_t sm = size_t(m);
    Staging S(d->stream.get());
    const double *d_chain = nullptr, *d_moments = nullptr, *d_q = nullptr, *d_d = nullptr, *d_x = nullptr;
    const uint8_t* d_valid = nullptr;
    double* d_out = nullptr;
    int32_t* d_corners = nullptr;
    if (const int rc = volume_upload(*g, *c, chain, valid, moments, v, S, d_chain, d_valid, d_moments)) return rc;
    if (const int rc = S.in(q6, sm * 6, "the receiver list", d_q)) return rc;
    if (const int rc = S.in(d3, sm * 3, "the receivers' directions", d_d)) return rc;
    if (const int rc = S.in(x, sm, "the receivers' exponents", d_x)) return rc;
    if (const int rc = S.out(out3, sm * 3, "the receivers' radiance", d_out)) return rc;
    if (const int rc = S.out(corners, sm, "the receivers' corners", d_corners)) return rc;
    launch_reflection_volume_lookup(volume_of(*g, *c, d_chain, d_valid, d_moments, v), d_q, d_d, d_x, m, d_out, d_corners, d->stream.get());
    return S.finish(launch_result());
}

int mcpt_baked_radiance_specular_device(mcpt_device* d, const mcpt_baked_source* s, const mcpt_baked_specular* sp, const double* d_rays6, int64_t n,
                                        int32_t flags, const mcpt_baked_outputs* o, const mcpt_baked_specular_outputs* so, mcpt_stats* stats, void* stream)
{
    if (const int rc = radiance_check(s, sp, d_rays6, n, flags, o, so)) return rc;
    if (const int rc = device_gate(d)) return rc;
    BakedSpecular spec{};
    spec.V = volume_of(*sp);
    if (so) spec.rays = BakedSpecOut{so->spec3, so->ks3, so->r3, so->ns, so->slit};
    return baked_radiance_device(d, *s, d_rays6, n, flags, *o, &spec, stats, static_cast<hipStream_t>(stream));
}

int mcpt_baked_radiance_specular(mcpt_device* d, const mcpt_baked_source* s, const mcpt_baked_specular* sp, const double* rays6, int64_t n, int32_t flags,
                                 const mcpt_baked_outputs* o, const mcpt_baked_specular_outputs* so, mcpt_stats* stats)
{
    if (const int rc = radiance_check(s, sp, rays6, n, flags, o, so)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    Staging S(d->stream.get());
    mcpt_baked_source src;
    if (const int rc = baked_source_upload(d, *s, S, src)) return rc;
    if (n == 0) return MCPT_OK;
    BakedSpecular spec{};
    {
        const double *d_chain = nullptr, *d_moments = nullptr;
        const uint8_t* d_valid = nullptr;
        if (const int rc = volume_upload(*sp->grid, *sp->chain, sp->chain_data, sp->valid, sp->moments, sp->visibility, S, d_chain, d_valid, d_moments)) return rc;
        spec.V = volume_of(*sp->grid, *sp->chain, d_chain, d_valid, d_moments, sp->visibility);
    }
    const size_t sn = size_t(n);
    const double* d_rays = nullptr;
    mcpt_baked_outputs dev{};
    if (const int rc = S.in(rays6, sn * 6, "the rays", d_rays)) return rc;
    // one device array per output the caller asks for.  The radiance is the plain call's with the specular term added in place: a caller
    // who asks for neither gets neither
    if (const int rc = S.out(o->radiance3, sn * 3, "a baked output", dev.radiance3)) return rc;
    if (const int rc = S.out(o->kind, sn, "a baked output", dev.kind)) return rc;
    if (const int rc = S.out(o->face, sn, "a baked output", dev.face)) return rc;
    if (const int rc = S.out(o->q6, sn * 6, "a baked output", dev.q6)) return rc;
    if (const int rc = S.out(o->uv2, sn * 2, "a baked output", dev.uv2)) return rc;
    if (const int rc = S.out(o->kd3, sn * 3, "a baked output", dev.kd3)) return rc;
    if (const int rc = S.out(o->e3, sn * 3, "a baked output", dev.e3)) return rc;
    if (const int rc = S.out(o->lit, sn, "a baked output", dev.lit)) return rc;
    if (so) {
        if (const int rc = S.out(so->spec3, sn * 3, "a baked specular output", spec.rays.spec3)) return rc;
        if (const int rc = S.out(so->ks3, sn * 3, "a baked specular output", spec.rays.ks3)) return rc;
        if (const int rc = S.out(so->r3, sn * 3, "a baked specular output", spec.rays.r3)) return rc;
        if (const int rc = S.out(so->ns, sn, "a baked specular output", spec.rays.ns)) return rc;
        if (const int rc = S.out(so->slit, sn, "a baked specular output", spec.rays.slit)) return rc;
    }
    return S.finish(baked_radiance_device(d, src, d_rays, n, flags, dev, &spec, stats, d->stream.get()));
}

int mcpt_render_baked_specular_device(mcpt_device* d, const mcpt_baked_source* s, const mcpt_baked_specular* sp, const mcpt_baked_frame_params* p,
                                      double* d_img, int32_t* d_counts3, int32_t* d_lit, int32_t* d_slit, mcpt_stats* stats, void* stream)
{
    if (const int rc = frame_check(s, sp, p, d_img)) return rc;
    if (const int rc = device_gate(d)) return rc;
    BakedSpecular spec{};
    spec.V = volume_of(*sp);
    spec.pixel_slit = d_slit;
    return baked_frame_device(d, *s, *p, d_img, d_counts3, d_lit, &spec, stats, static_cast<hipStream_t>(stream));
}

int mcpt_render_baked_specular(mcpt_device* d, const mcpt_baked_source* s, const mcpt_baked_specular* sp, const mcpt_baked_frame_params* p, double* img,
                               int32_t* counts3, int32_t* lit, int32_t* slit, mcpt_stats* stats)
{
    if (const int rc = frame_check(s, sp, p, img)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    Staging S(d->stream.get());
    mcpt_baked_source src;
    if (const int rc = baked_source_upload(d, *s, S, src)) return rc;
    const size_t px = size_t(d->width) * size_t(d->height);
    if (px == 0) return MCPT_OK;
    BakedSpecular spec{};
    {
        const double *d_chain = nullptr, *d_moments = nullptr;
        const uint8_t* d_valid = nullptr;
        if (const int rc = volume_upload(*sp->grid, *sp->chain, sp->chain_data, sp->valid, sp->moments, sp->visibility, S, d_chain, d_valid, d_moments)) return rc;
        spec.V = volume_of(*sp->grid, *sp->chain, d_chain, d_valid, d_moments, sp->visibility);
    }
    double* d_img = nullptr;
    int32_t *d_counts = nullptr, *d_lit = nullptr;
    if (const int rc = S.out(img, px * 3, "the frame", d_img)) return rc;
    if (const int rc = S.out(counts3, px * 3, "the frame's counts", d_counts)) return rc;
    if (const int rc = S.out(lit, px, "the frame's lookups", d_lit)) return rc;
    if (const int rc = S.out(slit, px, "the frame's specular lookups", spec.pixel_slit)) return rc;
    return S.finish(baked_frame_device(d, src, *p, d_img, d_counts, d_lit, &spec, stats, d->stream.get()));
}

}  // extern "C"
