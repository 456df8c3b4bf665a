// C ABI, reflection probes (include/mcpt.h: mcpt_reflection_texels, mcpt_bake_reflection*, mcpt_reflection_rays,
// mcpt_reflection_prefilter*, mcpt_reflection_lookup*): per probe an octahedral map of the incoming radiance, a chain of maps filtered
// from it with Phong lobes, and the lookup of a direction and an exponent in such a chain.  A bake draws the rays of a chunk of texels
// into a workspace the device keeps (reflection.hip), answers them with the unchanged query call (query_api.cpp: query_device, the ray
// kind, one sample per ray) and folds texel by texel.  The arithmetic is reflection.hpp's, compiled here for the host forms.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "chunks.hpp"
#include "handles.hpp"
#include "reflection.hpp"

using namespace mcpt;

static constexpr size_t kRayBytes = (6 + 3) * sizeof(double) + 2 * sizeof(int32_t);
static_assert(kRayBytes == 80, "mcpt.h states the workspace's bytes per ray");    // (the default workspace of 2^22 rays: 320 MB)

static int res_check(int32_t res)
{
    return res >= 1 && res <= kReflectionMaxRes ? MCPT_OK : fail(MCPT_ERR_ARG, "res must be in 1 .. 256");
}

// what every bake refuses of its parameters and its list, without looking at the list
static int params_check(const mcpt_reflection_params* p, int64_t n)
{
    if (!p) return fail(MCPT_ERR_ARG, "null reflection parameters");
    if (p->spp < 1) return fail(MCPT_ERR_ARG, "spp must be >= 1");
    if (p->sample_base < 0) return fail(MCPT_ERR_ARG, "sample_base must be >= 0");
    if (const int rc = res_check(p->res)) return rc;
    if (const int rc = flags_check(p->flags)) return rc;
    if (p->workspace_rays < 0) return fail(MCPT_ERR_ARG, "workspace_rays must be >= 0");
    for (int i = 0; i < 4; i++)
        if (p->reserved[i] != 0) return fail(MCPT_ERR_ARG, "mcpt_reflection_params.reserved must be 0");
    if (n < 0) return fail(MCPT_ERR_ARG, "the number of probes must be >= 0");
    // n * R^2 * S <= 2^31 - 1, without overflow: R^2 * S <= 2^47
    const int64_t per_probe = int64_t(p->res) * p->res * p->spp;
    if (n > 0 && (per_probe > kInt32Max || n > kInt32Max / per_probe)) return fail(MCPT_ERR_ARG, "probes * res * res * spp must not exceed 2^31 - 1");
    return MCPT_OK;
}
static int bake_check(const mcpt_reflection_params* p, int64_t n, const void* p3, const void* radiance)
{
    if (const int rc = params_check(p, n)) return rc;
    if (n > 0 && (!p3 || !radiance)) return fail(MCPT_ERR_ARG, "null probe list or radiance");
    return MCPT_OK;
}

// ... and what the host-pointer forms refuse of the list itself
static int list_check(const mcpt_reflection_params& p, const double* p3, const int32_t* id_base, int64_t n)
{
    const int64_t per_probe = int64_t(p.res) * p.res * p.spp;
    for (int64_t i = 0; i < n; i++) {
        for (int c = 0; c < 3; c++)
            if (!std::isfinite(p3[i * 3 + c])) return fail(MCPT_ERR_ARG, "probe " + std::to_string(i) + ": component that is not finite");
        if (id_base) {
            if (id_base[i] < 0) return fail(MCPT_ERR_ARG, "probe " + std::to_string(i) + ": negative id_base");
            if (int64_t(id_base[i]) + per_probe - 1 > kInt32Max)
                return fail(MCPT_ERR_ARG, "probe " + std::to_string(i) + ": id_base + res * res * spp - 1 must not exceed 2^31 - 1");
        }
    }
    return MCPT_OK;
}

// what every call refuses of a chain, in the struct's field order
int reflection_chain_check(const mcpt_reflection_chain* c)
{
    if (!c) return fail(MCPT_ERR_ARG, "null reflection chain");
    if (const int rc = res_check(c->res)) return rc;
    if (c->num_levels < 1 || c->num_levels > kReflectionMaxLevels) return fail(MCPT_ERR_ARG, "num_levels must be in 1 .. 8");
    for (int l = 0; l < kReflectionMaxLevels; l++) {
        const int32_t r = c->level_res[l];
        if (l < c->num_levels ? (r < 1 || r > kReflectionMaxRes) : r != 0)
            return fail(MCPT_ERR_ARG, "level_res must be in 1 .. 256 for every level and 0 beyond the last");
    }
    for (int l = 0; l < kReflectionMaxLevels; l++) {
        const int32_t e = c->level_ns[l];
        if (l >= c->num_levels ? e != 0 : (e < 0 || e > kReflectionMaxNs || (l > 0 && e >= c->level_ns[l - 1])))
            return fail(MCPT_ERR_ARG, "level_ns must be in 0 .. 65535, strictly descending, and 0 beyond the last level");
    }
    for (int i = 0; i < 4; i++)
        if (c->reserved[i] != 0) return fail(MCPT_ERR_ARG, "mcpt_reflection_chain.reserved must be 0");
    return MCPT_OK;
}

static int prefilter_check(const mcpt_reflection_chain* c, const void* radiance, int64_t n, const void* chain)
{
    if (const int rc = reflection_chain_check(c)) return rc;
    if (const int rc = count_check(n, "probes")) return rc;
    if (n > 0 && (!radiance || !chain)) return fail(MCPT_ERR_ARG, "null radiance or chain");
    return MCPT_OK;
}

static int lookup_check(const mcpt_reflection_chain* c, const void* chain, int64_t n, const void* probe, const void* d3, const void* x, int64_t m, const void* out3)
{
    if (const int rc = reflection_chain_check(c)) return rc;
    if (const int rc = count_check(n, "probes")) return rc;
    if (const int rc = count_check(m, "receivers")) return rc;
    if (m > 0 && (!chain || !probe || !d3 || !x || !out3)) return fail(MCPT_ERR_ARG, "null chain, probe indices, directions, exponents or radiance");
    return MCPT_OK;
}

int reflection_finite_check(const double* a, size_t count, const char* what)
{
    for (size_t i = 0; i < count; i++)
        if (!std::isfinite(a[i])) return fail(MCPT_ERR_ARG, std::string(what) + ": value " + std::to_string(i) + " is not finite");
    return MCPT_OK;
}

// ... and what the host-pointer forms of the lookup refuse of the arrays themselves
static int lookup_arrays_check(const mcpt_reflection_chain& c, const double* chain, int64_t n, const int32_t* probe, const double* d3, const double* x, int64_t m)
{
    if (const int rc = reflection_finite_check(chain, size_t(n) * size_t(reflection_chain_texels(c)) * 3, "the chain")) return rc;
    for (int64_t q = 0; q < m; q++) {
        const double* d = d3 + q * 3;
        const double l = (std::fabs(d[0]) + std::fabs(d[1])) + std::fabs(d[2]);
        if (!(l > 0.0 && std::isfinite(l))) return fail(MCPT_ERR_ARG, "receiver " + std::to_string(q) + ": direction not finite, zero, or too long");
        if (probe[q] < 0 || probe[q] >= n) return fail(MCPT_ERR_ARG, "receiver " + std::to_string(q) + ": probe index out of range");
        if (!(std::isfinite(x[q]) && x[q] >= 0.0)) return fail(MCPT_ERR_ARG, "receiver " + std::to_string(q) + ": the exponent must be finite and >= 0");
    }
    return MCPT_OK;
}

// the counters of one chunk's query added to the call's (not stats.cpp's add_piece: rays_primary and samples are the bake's own, set after
// its loop, and stay 0 in the statistics of a bake that fails)
static void add_stats(mcpt_stats& s, const mcpt_stats& q)
{
    s.rays_shadow += q.rays_shadow; s.rays_bounce += q.rays_bounce; s.node_visits += q.node_visits; s.tri_tests += q.tri_tests;
    s.shade_calls += q.shade_calls; s.shadow_skipped += q.shadow_skipped; s.dom_rays += q.dom_rays; s.dom_node_visits += q.dom_node_visits;
    s.dom_tri_tests += q.dom_tri_tests; s.ms_trace += q.ms_trace; s.ms_total += q.ms_total; s.launches += q.launches;
    s.max_depth = s.max_depth > q.max_depth ? s.max_depth : q.max_depth;
}

// The bake on st, after the refusals and the gate; device pointers throughout.  Nothing here waits for st unless the caller asks for
// statistics (the query call waits for the device's frames in flight, as every query does).
static int bake_device(mcpt_device* d, const double* d_p3, const int32_t* d_id_base, int64_t n, const mcpt_reflection_params& rp, double* d_radiance,
                       double* d_stderr, int32_t* d_hits, mcpt_stats* stats, hipStream_t st)
{
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return MCPT_OK;
    if (const int rc = motion_home(d)) return rc;           // a device that holds a motion answers from key 0
    if (const int rc = geometry_gate(d)) return rc;
    Lease l;
    if (const int rc = lease(d->refl, st, l)) return rc;    // the bake before this one has left the workspace
    mcpt_device::Reflection& w = *d->refl;
    const int64_t texels = n * rp.res * rp.res;             // <= 2^31 - 1 with spp
    const int64_t per_chunk = chunk_plan(rp.workspace_rays, rp.spp, texels);    // whole texels
    const size_t sr = size_t(per_chunk) * size_t(rp.spp);   // <= 2^31 - 1
    if (const int rc = grow(w.rays6, sr * 6, "the reflection rays")) return rc;
    if (const int rc = grow(w.mean, sr * 3, "the reflection samples' radiance")) return rc;
    if (const int rc = grow(w.ids, sr, "the reflection rays' ids")) return rc;
    if (const int rc = grow(w.hits, sr, "the reflection samples' hits")) return rc;
    int rc = MCPT_OK;
    for (int64_t first = 0; first < texels && rc == MCPT_OK; first += per_chunk) {
        ReflChunk c{};
        c.p3 = d_p3; c.id_base = d_id_base; c.R = rp.res; c.S = rp.spp; c.sample_base = rp.sample_base; c.seed = rp.seed;
        c.first_texel = first; c.texels = chunk_count(per_chunk, texels, first);
        c.rays6 = w.rays6.get(); c.ids = w.ids.get(); c.mean3 = w.mean.get(); c.hits = w.hits.get();
        const int64_t rays = c.texels * c.S;
        launch_reflection_rays(c, nullptr, rays, st);
        if ((rc = launch_result()) != MCPT_OK) break;
        mcpt_stats qs;
        rc = query_device(d, DQuery{w.rays6.get(), MCPT_QUERY_RAY, w.mean.get(), nullptr, w.hits.get()}, w.ids.get(), rays, 1, rp.sample_base, rp.seed,
                          rp.flags, stats ? &qs : nullptr, st);
        if (rc != MCPT_OK) break;
        if (stats) add_stats(*stats, qs);
        launch_reflection_fold(c, d_radiance, d_stderr, d_hits, st);
        rc = launch_result();
    }
    if ((rc = l.end(rc)) != MCPT_OK) return rc;
    if (stats) {
        HIP_TRY(hipStreamSynchronize(st));
        stats->rays_primary = stats->samples = uint64_t(texels) * uint64_t(rp.spp);
    }
    return MCPT_OK;
}

extern "C" {

int mcpt_reflection_texels(int32_t res, double* d3, double* w)
{
    if (const int rc = res_check(res)) return rc;
    for (int b = 0; b < res * res; b++) {
        double d[3], o;
        reflection_texel(res, b, d, o);
        if (d3) for (int c = 0; c < 3; c++) d3[size_t(b) * 3 + size_t(c)] = d[c];
        if (w) w[b] = o;
    }
    return MCPT_OK;
}

int mcpt_bake_reflection_device(mcpt_device* d, const double* d_p3, const int32_t* d_id_base, int64_t n, const mcpt_reflection_params* p, double* d_radiance,
                                double* d_stderr, int32_t* d_hits, mcpt_stats* stats, void* stream)
{
    if (const int rc = bake_check(p, n, d_p3, d_radiance)) return rc;
    if (const int rc = device_gate(d)) return rc;
    return bake_device(d, d_p3, d_id_base, n, *p, d_radiance, d_stderr, d_hits, stats, static_cast<hipStream_t>(stream));
}

int mcpt_bake_reflection(mcpt_device* d, const double* p3, const int32_t* id_base, int64_t n, const mcpt_reflection_params* p, double* radiance, double* stderr3,
                         int32_t* hits, mcpt_stats* stats)
{
    if (const int rc = bake_check(p, n, p3, radiance)) return rc;
    if (const int rc = list_check(*p, p3, id_base, n)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return MCPT_OK;
    const size_t sn = size_t(n), texels = sn * size_t(p->res) * size_t(p->res);
    Staging S(d->stream.get());
    const double* d_p = nullptr;
    const int32_t* d_base = nullptr;
    double *d_rad = nullptr, *d_err = nullptr;
    int32_t* d_hits = nullptr;
    if (const int rc = S.in(p3, sn * 3, "the probe list", d_p)) return rc;
    if (const int rc = S.in(id_base, sn, "the probes' id bases", d_base)) return rc;
    if (const int rc = S.out(radiance, texels * 3, "the probes' radiance", d_rad)) return rc;
    if (const int rc = S.out(stderr3, texels * 3, "the probes' standard errors", d_err)) return rc;
    if (const int rc = S.out(hits, texels, "the probes' hits", d_hits)) return rc;
    return S.finish(bake_device(d, d_p, d_base, n, *p, d_rad, d_err, d_hits, stats, d->stream.get()));
}

int mcpt_reflection_rays(mcpt_device* d, const double* p3, const int32_t* id_base, int64_t n, const mcpt_reflection_params* p, const int64_t* entry, int64_t m,
                         double* rays6, int32_t* ids)
{
    if (const int rc = params_check(p, n)) return rc;
    if (const int rc = count_check(m, "entries")) return rc;
    if (m > 0 && (!p3 || !entry || !rays6 || !ids)) return fail(MCPT_ERR_ARG, "null argument");
    const int64_t entries = n * p->res * p->res * p->spp;
    for (int64_t i = 0; i < m; i++)
        if (entry[i] < 0 || entry[i] >= entries) return fail(MCPT_ERR_ARG, "entry " + std::to_string(i) + ": outside 0 .. probes * res * res * spp - 1");
    if (m > 0)
        if (const int rc = list_check(*p, p3, id_base, n)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (m == 0) return MCPT_OK;
    const size_t sn = size_t(n), sm = size_t(m);
    Staging S(d->stream.get());
    ReflChunk c{};
    const long long* d_entry = nullptr;
    static_assert(sizeof(long long) == sizeof(int64_t), "the entry list is int64");
    if (const int rc = S.in(p3, sn * 3, "the probe list", c.p3)) return rc;
    if (const int rc = S.in(id_base, sn, "the probes' id bases", c.id_base)) return rc;
    if (const int rc = S.in(reinterpret_cast<const long long*>(entry), sm, "the entries", d_entry)) return rc;
    if (const int rc = S.out(rays6, sm * 6, "the entries' rays", c.rays6)) return rc;
    if (const int rc = S.out(ids, sm, "the entries' ids", c.ids)) return rc;
    c.R = p->res; c.S = p->spp; c.sample_base = p->sample_base; c.seed = p->seed;
    launch_reflection_rays(c, d_entry, m, d->stream.get());
    return S.finish(launch_result());
}

int mcpt_reflection_prefilter_host(const mcpt_reflection_chain* c, const double* radiance, int64_t n, double* chain)
{
    if (const int rc = prefilter_check(c, radiance, n, chain)) return rc;
    if (n == 0) return MCPT_OK;
    const int src = c->res * c->res, T = reflection_chain_texels(*c);
    if (const int rc = reflection_finite_check(radiance, size_t(n) * size_t(src) * 3, "the radiance")) return rc;
    std::vector<double> dw(size_t(src) * 4);                // the source texels' directions and solid angles, as the kernel's records hold them
    for (int b = 0; b < src; b++) reflection_texel(c->res, b, &dw[size_t(b) * 4], dw[size_t(b) * 4 + 3]);
    for (int l = 0, first = 0; l < c->num_levels; first += c->level_res[l] * c->level_res[l], l++)
        for (int o = 0; o < c->level_res[l] * c->level_res[l]; o++) {
            double r[3], w;
            reflection_texel(c->level_res[l], o, r, w);
            for (int64_t i = 0; i < n; i++)
                reflection_filter(dw.data(), radiance + size_t(i) * size_t(src) * 3, src, r, c->level_ns[l], chain + (size_t(i) * size_t(T) + size_t(first + o)) * 3);
        }
    return MCPT_OK;
}

int mcpt_reflection_prefilter_device(mcpt_device* d, const mcpt_reflection_chain* c, const double* d_radiance, int64_t n, double* d_chain, void* stream)
{
    if (const int rc = prefilter_check(c, d_radiance, n, d_chain)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (n == 0) return MCPT_OK;
    launch_reflection_prefilter(*c, d_radiance, n, d_chain, static_cast<hipStream_t>(stream));
    return launch_result();
}

int mcpt_reflection_prefilter(mcpt_device* d, const mcpt_reflection_chain* c, const double* radiance, int64_t n, double* chain)
{
    if (const int rc = prefilter_check(c, radiance, n, chain)) return rc;
    if (n > 0)
        if (const int rc = reflection_finite_check(radiance, size_t(n) * size_t(c->res) * size_t(c->res) * 3, "the radiance")) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (n == 0) return MCPT_OK;
    const size_t in = size_t(n) * size_t(c->res) * size_t(c->res) * 3, out = size_t(n) * size_t(reflection_chain_texels(*c)) * 3;
    Staging S(d->stream.get());
    const double* d_rad = nullptr;
    double* d_chain = nullptr;
    if (const int rc = S.in(radiance, in, "the probes' radiance", d_rad)) return rc;
    if (const int rc = S.out(chain, out, "the probes' chains", d_chain)) return rc;
    launch_reflection_prefilter(*c, d_rad, n, d_chain, d->stream.get());
    return S.finish(launch_result());
}

int mcpt_reflection_lookup_host(const mcpt_reflection_chain* c, const double* chain, int64_t n, const int32_t* probe, const double* d3, const double* x,
                                int64_t m, double* out3)
{
    if (const int rc = lookup_check(c, chain, n, probe, d3, x, m, out3)) return rc;
    if (m == 0) return MCPT_OK;
    if (const int rc = lookup_arrays_check(*c, chain, n, probe, d3, x, m)) return rc;
    const size_t T = size_t(reflection_chain_texels(*c));
    for (int64_t q = 0; q < m; q++) reflection_lookup(*c, chain + size_t(probe[q]) * T * 3, d3 + q * 3, x[q], out3 + q * 3);
    return MCPT_OK;
}

int mcpt_reflection_lookup_device(mcpt_device* d, const mcpt_reflection_chain* c, const double* d_chain, int64_t n, const int32_t* d_probe, const double* d_d3,
                                  const double* d_x, int64_t m, double* d_out3, void* stream)
{
    if (const int rc = lookup_check(c, d_chain, n, d_probe, d_d3, d_x, m, d_out3)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (m == 0) return MCPT_OK;
    launch_reflection_lookup(*c, d_chain, n, d_probe, d_d3, d_x, m, d_out3, static_cast<hipStream_t>(stream));
    return launch_result();
}

int mcpt_reflection_lookup(mcpt_device* d, const mcpt_reflection_chain* c, const double* chain, int64_t n, const int32_t* probe, const double* d3,
                           const double* x, int64_t m, double* out3)
{
    if (const int rc = lookup_check(c, chain, n, probe, d3, x, m, out3)) return rc;
    if (m > 0)
        if (const int rc = lookup_arrays_check(*c, chain, n, probe, d3, x, m)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (m == 0) return MCPT_OK;
    const size_t sm = size_t(m), texels = size_t(n) * size_t(reflection_chain_texels(*c));
    Staging S(d->stream.get());
    const double *d_chain = nullptr, *d_d = nullptr, *d_x = nullptr;
    const int32_t* d_probe = nullptr;
    double* d_out = nullptr;
    if (const int rc = S.in(chain, texels * 3, "the probes' chains", d_chain)) return rc;
    if (const int rc = S.in(probe, sm, "the receivers' probes", d_probe)) return rc;
    if (const int rc = S.in(d3, sm * 3, "the receivers' directions", d_d)) return rc;
    if (const int rc = S.in(x, sm, "the receivers' exponents", d_x)) return rc;
    if (const int rc = S.out(out3, sm * 3, "the receivers' radiance", d_out)) return rc;
    launch_reflection_lookup(*c, d_chain, n, d_probe, d_d, d_x, m, d_out, d->stream.get());
    return S.finish(launch_result());
}

}  // extern "C"
