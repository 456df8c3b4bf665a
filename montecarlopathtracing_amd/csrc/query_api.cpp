// C ABI, radiance queries (include/mcpt.h: mcpt_query_radiance*, mcpt_query_rays): the integrator behind a caller's list of rays or
// surface points.  The list is the sample source of an ordinary render call (render.cpp: the per-sample route with a query pass for the
// camera pass and the query fold for the frame's), so chunking, engines, hand-over and statistics are the frame's own.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>
#include <string>

#include "handles.hpp"

using namespace mcpt;

static int kind_check(int32_t kind)
{
    return kind == MCPT_QUERY_RAY || kind == MCPT_QUERY_HEMISPHERE ? MCPT_OK : fail(MCPT_ERR_ARG, "unknown query kind");
}

// what every query call refuses of its sample range and count, and of its flags: the pieces of query_params_check and sh_params_check, which
// refuse the same things in the same order (lightmap_api.cpp shares them: handles.hpp)
int range_check(int32_t spp, int32_t sample_base, int64_t n)
{
    if (spp < 1) return fail(MCPT_ERR_ARG, "spp must be >= 1");
    if (sample_base < 0) return fail(MCPT_ERR_ARG, "sample_base must be >= 0");
    if (int64_t(sample_base) + int64_t(spp) > kInt32Max) return fail(MCPT_ERR_ARG, "sample_base + spp must not exceed 2^31 - 1");
    return count_check(n, "queries");
}
int flags_check(int32_t flags)
{
    return flags == 0 || flags == MCPT_RENDER_MEGAKERNEL ? MCPT_OK : fail(MCPT_ERR_ARG, "unknown query flag (0 or MCPT_RENDER_MEGAKERNEL)");
}

// what both forms of mcpt_query_radiance refuse without looking at the list
int query_params_check(const mcpt_query_params* p, int64_t n, const void* q6, const void* mean3)
{
    if (!p) return fail(MCPT_ERR_ARG, "null query parameters");
    if (const int rc = range_check(p->spp, p->sample_base, n)) return rc;
    if (const int rc = kind_check(p->kind)) return rc;
    if (const int rc = flags_check(p->flags)) return rc;
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(MCPT_ERR_ARG, "mcpt_query_params.reserved must be 0");
    if (n > 0 && (!q6 || !mean3)) return fail(MCPT_ERR_ARG, "null query list or mean");
    return MCPT_OK;
}
// ... and both forms of mcpt_query_sh
int sh_params_check(const mcpt_sh_params* p, int64_t n, const void* p3, const void* sh27)
{
    if (!p) return fail(MCPT_ERR_ARG, "null probe parameters");
    if (const int rc = range_check(p->spp, p->sample_base, n)) return rc;
    if (const int rc = flags_check(p->flags)) return rc;
    if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0) return fail(MCPT_ERR_ARG, "mcpt_sh_params.reserved must be 0");
    if (n > 0 && (!p3 || !sh27)) return fail(MCPT_ERR_ARG, "null probe list or coefficients");
    return MCPT_OK;
}

// what the host-pointer forms refuse of the list itself
int query_list_check(const double* q6, const int32_t* ids, int64_t n, int32_t kind)
{
    for (int64_t i = 0; i < n; i++) {
        if (ids && ids[i] < 0) return fail(MCPT_ERR_ARG, "query " + std::to_string(i) + ": negative id");
        const double* q = q6 + i * 6;
        for (int c = 0; c < 6; c++)
            if (!std::isfinite(q[c])) return fail(MCPT_ERR_ARG, "query " + std::to_string(i) + ": component that is not finite");
        const double l2 = (q[3] * q[3] + q[4] * q[4]) + q[5] * q[5];
        if (kind == MCPT_QUERY_RAY) {
            if (!(std::fabs(l2 - 1.0) <= 1e-9)) return fail(MCPT_ERR_ARG, "query " + std::to_string(i) + ": the direction must have unit length");
        } else {
            const double l = std::sqrt(l2);
            if (!(std::isfinite(l) && l > 0.0)) return fail(MCPT_ERR_ARG, "query " + std::to_string(i) + ": the normal must have a non-zero finite length");
        }
    }
    return MCPT_OK;
}

// ... and of a probe list
int probe_list_check(const double* p3, const int32_t* ids, int64_t n)
{
    for (int64_t i = 0; i < n; i++) {
        if (ids && ids[i] < 0) return fail(MCPT_ERR_ARG, "probe " + std::to_string(i) + ": negative id");
        for (int c = 0; c < 3; c++)
            if (!std::isfinite(p3[i * 3 + c])) return fail(MCPT_ERR_ARG, "probe " + std::to_string(i) + ": component that is not finite");
    }
    return MCPT_OK;
}

// The call itself, after the refusals: q's list, of q.kind, as the sample source of a render call on `stream`.
int query_device(mcpt_device* d, const DQuery& q, const int32_t* d_ids, int64_t n, int32_t spp, int32_t sample_base, uint64_t seed, int32_t flags,
                 mcpt_stats* stats, void* stream)
{
    if (const int rc = device_gate(d)) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return MCPT_OK;
    if (const int rc = motion_home(d)) return rc;           // a device that holds a motion answers from key 0
    if (const int rc = geometry_gate(d)) return rc;
    if (const int rc = wait_for_frames(d)) return rc;       // the call uses frame slot 0 and the device's look stream
    mcpt_render_params rp{};
    rp.spp = spp; rp.seed = seed; rp.world = 1; rp.flags = flags;
    SampleRange r{sample_base, spp, spp, nullptr, nullptr, nullptr, nullptr, d->env.get()};
    r.query = &q;
    // a call that fails half-way must not leave half-recorded event pairs behind (render.cpp: mcpt_render_device)
    const size_t ev_used0 = d->ev_used;
    int slot_used = -1;
    const int rc = render_device_impl(d, r, PixelList{d_ids, n}, &rp, nullptr, stats, static_cast<hipStream_t>(stream), slot_used);
    if (rc != MCPT_OK) d->ev_used = ev_used0;
    return rc;
}

// The host-pointer form of a call whose list, of `kind`, has `in` doubles per entry and whose answers have `out`: the caller's arrays are pageable host
// memory, so blocking copies on either side of the device form, which itself is ordered on d->stream.
static int query_host(mcpt_device* d, int kind, int in, int out, const double* list, const int32_t* ids, int64_t n, int32_t spp,
                      int32_t sample_base, uint64_t seed, int32_t flags, double* mean, double* err, int32_t* hits, mcpt_stats* stats)
{
    if (const int rc = device_gate(d)) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return MCPT_OK;
    const size_t sn = size_t(n);
    Staging S(d->stream.get());
    const int32_t* d_ids = nullptr;
    DQuery q{nullptr, kind, nullptr, nullptr, nullptr};
    if (const int rc = S.in(list, sn * in, "the query list", q.q6)) return rc;
    if (const int rc = S.in(ids, sn, "the queries' ids", d_ids)) return rc;
    if (const int rc = S.out(mean, sn * out, "the queries' answers", q.mean3)) return rc;
    if (const int rc = S.out(err, sn * out, "the queries' standard errors", q.stderr3)) return rc;
    if (const int rc = S.out(hits, sn, "the queries' hits", q.hits)) return rc;
    return S.finish(query_device(d, q, d_ids, n, spp, sample_base, seed, flags, stats, d->stream.get()));
}

// the rays of a list on the host: the body of mcpt_query_rays and mcpt_query_sh_rays after their refusals (`in` doubles per entry)
static int rays_host(mcpt_device* d, int kind, int in, const double* list, const int32_t* ids, int64_t n, uint64_t seed, const int32_t* k, double* rays6)
{
    if (const int rc = device_gate(d)) return rc;
    if (n == 0) return MCPT_OK;
    const size_t sn = size_t(n);
    Staging S(d->stream.get());
    const int32_t *d_ids = nullptr, *d_k = nullptr;
    DQuery q{nullptr, kind, nullptr, nullptr, nullptr};
    double* d_rays = nullptr;
    if (const int rc = S.in(list, sn * in, "the query list", q.q6)) return rc;
    if (const int rc = S.in(k, sn, "the queries' sample indices", d_k)) return rc;
    if (const int rc = S.in(ids, sn, "the queries' ids", d_ids)) return rc;
    if (const int rc = S.out(rays6, sn * 6, "the queries' rays", d_rays)) return rc;
    launch_query_rays(q, seed, d_ids, d_k, n, d_rays, d->stream.get());
    return S.finish(launch_result());
}

extern "C" {

int mcpt_query_radiance_device(mcpt_device* d, const double* d_q6, const int32_t* d_ids, int64_t n, const mcpt_query_params* p, double* d_mean3,
                               double* d_stderr3, int32_t* d_hits, mcpt_stats* stats, void* stream)
{
    if (const int rc = query_params_check(p, n, d_q6, d_mean3)) return rc;
    return query_device(d, DQuery{d_q6, p->kind, d_mean3, d_stderr3, d_hits}, d_ids, n, p->spp, p->sample_base, p->seed, p->flags, stats, stream);
}

int mcpt_query_radiance(mcpt_device* d, const double* q6, const int32_t* ids, int64_t n, const mcpt_query_params* p, double* mean3, double* stderr3,
                        int32_t* hits, mcpt_stats* stats)
{
    if (const int rc = query_params_check(p, n, q6, mean3)) return rc;
    if (const int rc = query_list_check(q6, ids, n, p->kind)) return rc;
    return query_host(d, p->kind, 6, 3, q6, ids, n, p->spp, p->sample_base, p->seed, p->flags, mean3, stderr3,
                      hits, stats);
}

int mcpt_query_rays(mcpt_device* d, const double* q6, const int32_t* ids, int64_t n, uint64_t seed, int32_t kind, const int32_t* k, double* rays6)
{
    if (const int rc = count_check(n, "queries")) return rc;
    if (const int rc = kind_check(kind)) return rc;
    if (n > 0 && (!q6 || !k || !rays6)) return fail(MCPT_ERR_ARG, "null argument");
    for (int64_t i = 0; i < n; i++)
        if (k[i] < 0) return fail(MCPT_ERR_ARG, "query " + std::to_string(i) + ": negative sample index");
    if (const int rc = query_list_check(q6, ids, n, kind)) return rc;
    return rays_host(d, kind, 6, q6, ids, n, seed, k, rays6);
}

// ---- light probes: the same calls over a list of positions, whose samples leave uniformly over the sphere (query.hpp) and fold into nine
// spherical-harmonic coefficients per channel (query.hip: k_query_fold_sh)
int mcpt_query_sh_device(mcpt_device* d, const double* d_p3, const int32_t* d_ids, int64_t n, const mcpt_sh_params* p, double* d_sh27, double* d_stderr27,
                         int32_t* d_hits, mcpt_stats* stats, void* stream)
{
    if (const int rc = sh_params_check(p, n, d_p3, d_sh27)) return rc;
    return query_device(d, DQuery{d_p3, MCPT_QUERY_KIND_SPHERE, d_sh27, d_stderr27, d_hits}, d_ids, n, p->spp, p->sample_base, p->seed, p->flags, stats,
                        stream);
}

int mcpt_query_sh(mcpt_device* d, const double* p3, const int32_t* ids, int64_t n, const mcpt_sh_params* p, double* sh27, double* stderr27, int32_t* hits,
                  mcpt_stats* stats)
{
    if (const int rc = sh_params_check(p, n, p3, sh27)) return rc;
    if (const int rc = probe_list_check(p3, ids, n)) return rc;
    return query_host(d, MCPT_QUERY_KIND_SPHERE, 3, 27, p3, ids, n, p->spp, p->sample_base, p->seed, p->flags,
                      sh27, stderr27, hits, stats);
}

int mcpt_query_sh_rays(mcpt_device* d, const double* p3, const int32_t* ids, int64_t n, uint64_t seed, const int32_t* k, double* rays6)
{
    if (const int rc = count_check(n, "queries")) return rc;
    if (n > 0 && (!p3 || !k || !rays6)) return fail(MCPT_ERR_ARG, "null argument");
    for (int64_t i = 0; i < n; i++)
        if (k[i] < 0) return fail(MCPT_ERR_ARG, "probe " + std::to_string(i) + ": negative sample index");
    if (const int rc = probe_list_check(p3, ids, n)) return rc;
    return rays_host(d, MCPT_QUERY_KIND_SPHERE, 3, p3, ids, n, seed, k, rays6);
}

}  // extern "C"
