// C ABI, probe visibility (include/mcpt.h: mcpt_visibility_bin, mcpt_query_visibility*, mcpt_bake_volume_visibility*,
// mcpt_volume_irradiance_visible*): per probe an octahedral map of depth moments and the count of back-face hits, and the irradiance
// volume's lookup weighted by them.  A bake draws the probe query's own rays into a workspace the device keeps (visibility.hip), answers
// them with the unchanged closest-hit launch (hit_work.hpp: trace_leaf -- mcpt_trace_closest_device's walks, handing back the leaf, whose
// record holds the face normal) and folds chunk by chunk (hit_work.hpp: chunk_run).  The arithmetic is visibility.hpp's, compiled here for the host forms.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>
#include <string>

#include "chunks.hpp"
#include "handles.hpp"
#include "visibility.hpp"

using namespace mcpt;

// (the default workspace of 2^22 rays is 352 MB: 64 probes' worth of 65 536 samples, 65 536 probes' of 64)
static constexpr size_t kRayBytes = (6 + 1 + 3) * sizeof(double) + sizeof(int32_t);

// what every bake refuses of its parameters and its list, without looking at the list
static int bake_check(const mcpt_visibility_params* p, int64_t n, const void* p3, const void* moments)
{
    if (!p) return fail(MCPT_ERR_ARG, "null visibility parameters");
    if (p->spp < 1) return fail(MCPT_ERR_ARG, "spp must be >= 1");
    if (p->sample_base < 0) return fail(MCPT_ERR_ARG, "sample_base must be >= 0");
    if (int64_t(p->sample_base) + int64_t(p->spp) > kInt32Max) return fail(MCPT_ERR_ARG, "sample_base + spp must not exceed 2^31 - 1");
    if (p->res < 1 || p->res > 16) return fail(MCPT_ERR_ARG, "res must be in 1 .. 16");
    if (!(std::isfinite(p->max_distance) && p->max_distance > 0.0)) return fail(MCPT_ERR_ARG, "max_distance must be finite and > 0");
    if (!(std::isfinite(p->max_back_fraction) && p->max_back_fraction >= 0.0 && p->max_back_fraction <= 1.0))
        return fail(MCPT_ERR_ARG, "max_back_fraction must be in [0, 1]");
    if (p->workspace_rays < 0) return fail(MCPT_ERR_ARG, "workspace_rays must be >= 0");
    if (p->reserved0 != 0 || p->reserved[0] != 0 || p->reserved[1] != 0) return fail(MCPT_ERR_ARG, "mcpt_visibility_params.reserved must be 0");
    if (const int rc = count_check(n, "probes")) return rc;
    if (n > 0 && (!p3 || !moments)) return fail(MCPT_ERR_ARG, "null probe list or moments");
    return MCPT_OK;
}

// what every visibility-weighted lookup refuses of its knobs, in the struct's field order
int volume_visibility_check(const mcpt_volume_visibility* v)
{
    if (!v) return fail(MCPT_ERR_ARG, "null volume visibility");
    if (v->res < 1 || v->res > 16) return fail(MCPT_ERR_ARG, "res must be in 1 .. 16");
    if (v->flags != 0) return fail(MCPT_ERR_ARG, "mcpt_volume_visibility.flags must be 0");
    if (!(std::isfinite(v->max_distance) && v->max_distance > 0.0)) return fail(MCPT_ERR_ARG, "max_distance must be finite and > 0");
    if (!(std::isfinite(v->normal_bias) && v->normal_bias >= 0.0)) return fail(MCPT_ERR_ARG, "normal_bias must be finite and >= 0");
    if (!(std::isfinite(v->min_visibility) && v->min_visibility >= 0.0 && v->min_visibility <= 1.0))
        return fail(MCPT_ERR_ARG, "min_visibility must be in [0, 1]");
    for (int i = 0; i < 4; i++)
        if (v->reserved[i] != 0) return fail(MCPT_ERR_ARG, "mcpt_volume_visibility.reserved must be 0");
    return MCPT_OK;
}

// what every form of the lookup refuses without looking at the arrays
static int lookup_check(const mcpt_volume_grid* g, const mcpt_volume_visibility* v, const void* sh27, const void* moments, const void* q6, int64_t n,
                        const void* e3)
{
    if (const int rc = volume_grid_check(g)) return rc;
    if (const int rc = volume_visibility_check(v)) return rc;
    if (const int rc = count_check(n, "receivers")) return rc;
    if (n > 0 && (!sh27 || !moments || !q6 || !e3)) return fail(MCPT_ERR_ARG, "null coefficients, moments, receiver list or irradiance");
    return MCPT_OK;
}

// ... and what the host-pointer forms refuse of the arrays themselves
static int lookup_arrays_check(const mcpt_volume_grid& g, const mcpt_volume_visibility& v, const double* sh27, const double* moments, const double* q6, int64_t n)
{
    if (const int rc = volume_arrays_check(g, sh27, q6, n)) return rc;
    const int64_t bins = int64_t(v.res) * v.res, entries = volume_probes(g) * bins;
    for (int64_t i = 0; i < entries; i++) {
        const double mu = moments[i * 2], m2 = moments[i * 2 + 1];
        const bool data = std::isfinite(mu) && std::isfinite(m2) && mu >= 0.0, none = mu == -1.0 && m2 == 0.0;
        if (!data && !none)
            return fail(MCPT_ERR_ARG, "probe " + std::to_string(i / bins) + ", bin " + std::to_string(i % bins) + ": a moment that is neither finite with a mean >= 0 nor (-1, 0)");
    }
    return MCPT_OK;
}

// The bake on st, after the refusals; device pointers throughout.  Nothing here waits for st unless the caller asks for statistics.
static int bake_device(mcpt_device* d, const double* d_p3, const int32_t* d_ids, int64_t n, const mcpt_visibility_params& vp, double* d_moments,
                       int32_t* d_hits, int32_t* d_back, uint8_t* d_valid, mcpt_stats* stats, hipStream_t st)
{
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return MCPT_OK;
    if (const int rc = motion_home(d)) return rc;           // a device that holds a motion answers from key 0
    if (const int rc = geometry_gate(d)) return rc;
    Lease l;
    if (const int rc = lease(d->vis, st, l)) return rc;     // the bake before this one has left the workspace
    HitWork& w = *d->vis;
    const int64_t per_chunk = chunk_plan(vp.workspace_rays, vp.spp, n);     // whole probes
    if (const int rc = hit_work_grow(w, per_chunk * vp.spp, int64_t(1) << 40, "visibility", true)) return rc;
    static_assert(kRayBytes == 84, "mcpt.h states the workspace's bytes per ray");
    return chunk_run(n, per_chunk, vp.spp, l, stats, st, [&](int64_t first, int64_t count) {
        const RayChunk c{d_p3, d_ids, first, count, vp.spp, vp.sample_base, vp.seed, w.rays6.get(), w.leaf.get(), w.t.get()};
        launch_visibility_rays(c, st);
        trace_leaf(d, c.rays6, c.count * c.spp, c.leaf, c.t, w.p.get(), st);
        launch_visibility_fold(d->ds, c, vp, d_moments, d_hits, d_back, d_valid, st);
        return launch_result();
    });
}

// the grid form on st: the grid's positions into the volume's own list (volume_api.cpp), then the list form
static int bake_grid_device(mcpt_device* d, const mcpt_volume_grid& g, const mcpt_visibility_params& vp, double* d_moments, int32_t* d_hits, int32_t* d_back,
                            uint8_t* d_valid, mcpt_stats* stats, hipStream_t st)
{
    Lease l;
    if (const int rc = volume_points_device(d, g, st, l)) return rc;
    return l.end(bake_device(d, d->vol->p3.get(), nullptr, volume_probes(g), vp, d_moments, d_hits, d_back, d_valid, stats, st));
}

// A host-pointer bake of n probes: device copies of the answers around run(d_moments, d_hits, d_back, d_valid) on the device's stream
template <class Run>
static int bake_host(Staging& S, int64_t n, int res, double* moments, int32_t* hits, int32_t* back, uint8_t* valid, const Run& run)
{
    const size_t sn = size_t(n);
    double* d_m = nullptr;
    int32_t *d_hits = nullptr, *d_back = nullptr;
    uint8_t* d_valid = nullptr;
    if (const int rc = S.out(moments, sn * size_t(res) * size_t(res) * 2, "the probes' moments", d_m)) return rc;
    if (const int rc = S.out(hits, sn, "the probes' hits", d_hits)) return rc;
    if (const int rc = S.out(back, sn, "the probes' back-face hits", d_back)) return rc;
    if (const int rc = S.out(valid, sn, "the probes' validity", d_valid)) return rc;
    return S.finish(run(d_m, d_hits, d_back, d_valid));
}

extern "C" {

int mcpt_visibility_bin(const double* d3, int64_t n, int32_t res, int32_t* bin)
{
    if (n < 0) return fail(MCPT_ERR_ARG, "the number of directions must be >= 0");
    if (n > 0 && (!d3 || !bin)) return fail(MCPT_ERR_ARG, "null directions or bins");
    if (res < 1 || res > 16) return fail(MCPT_ERR_ARG, "res must be in 1 .. 16");
    for (int64_t i = 0; i < n; i++) {
        const double* v = d3 + i * 3;
        const double l = (std::fabs(v[0]) + std::fabs(v[1])) + std::fabs(v[2]);
        if (!(l > 0.0 && std::isfinite(l))) return fail(MCPT_ERR_ARG, "direction " + std::to_string(i) + ": not finite, zero, or too long");
    }
    for (int64_t i = 0; i < n; i++) bin[i] = visibility_bin(d3[i * 3], d3[i * 3 + 1], d3[i * 3 + 2], res);
    return MCPT_OK;
}

int mcpt_query_visibility_device(mcpt_device* d, const double* d_p3, const int32_t* d_ids, int64_t n, const mcpt_visibility_params* p, double* d_moments,
                                 int32_t* d_hits, int32_t* d_back, uint8_t* d_valid, mcpt_stats* stats, void* stream)
{
    if (const int rc = bake_check(p, n, d_p3, d_moments)) return rc;
    if (const int rc = device_gate(d)) return rc;
    return bake_device(d, d_p3, d_ids, n, *p, d_moments, d_hits, d_back, d_valid, stats, static_cast<hipStream_t>(stream));
}

int mcpt_query_visibility(mcpt_device* d, const double* p3, const int32_t* ids, int64_t n, const mcpt_visibility_params* p, double* moments, int32_t* hits,
                          int32_t* back, uint8_t* valid, mcpt_stats* stats)
{
    if (const int rc = bake_check(p, n, p3, moments)) return rc;
    if (const int rc = probe_list_check(p3, ids, n)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return MCPT_OK;
    Staging S(d->stream.get());
    const double* d_p = nullptr;
    const int32_t* d_ids = nullptr;
    if (const int rc = S.in(p3, size_t(n) * 3, "the probe list", d_p)) return rc;
    if (const int rc = S.in(ids, size_t(n), "the probes' ids", d_ids)) return rc;
    return bake_host(S, n, p->res, moments, hits, back, valid, [&](double* m, int32_t* h, int32_t* b, uint8_t* v) {
        return bake_device(d, d_p, d_ids, n, *p, m, h, b, v, stats, d->stream.get());
    });
}

int mcpt_bake_volume_visibility_device(mcpt_device* d, const mcpt_volume_grid* g, const mcpt_visibility_params* p, double* d_moments, int32_t* d_hits,
                                       int32_t* d_back, uint8_t* d_valid, mcpt_stats* stats, void* stream)
{
    if (!g || !p) return fail(MCPT_ERR_ARG, "null volume grid or visibility parameters");
    if (const int rc = volume_grid_check(g)) return rc;
    if (const int rc = bake_check(p, volume_probes(*g), g, d_moments)) return rc;
    if (const int rc = device_gate(d)) return rc;
    return bake_grid_device(d, *g, *p, d_moments, d_hits, d_back, d_valid, stats, static_cast<hipStream_t>(stream));
}

int mcpt_bake_volume_visibility(mcpt_device* d, const mcpt_volume_grid* g, const mcpt_visibility_params* p, double* moments, int32_t* hits, int32_t* back,
                                uint8_t* valid, mcpt_stats* stats)
{
    if (!g || !p) return fail(MCPT_ERR_ARG, "null volume grid or visibility parameters");
    if (const int rc = volume_grid_check(g)) return rc;
    if (const int rc = bake_check(p, volume_probes(*g), g, moments)) return rc;
    if (const int rc = device_gate(d)) return rc;
    Staging S(d->stream.get());
    return bake_host(S, volume_probes(*g), p->res, moments, hits, back, valid, [&](double* m, int32_t* h, int32_t* b, uint8_t* v) {
        return bake_grid_device(d, *g, *p, m, h, b, v, stats, d->stream.get());
    });
}

int mcpt_volume_irradiance_visible_host(const mcpt_volume_grid* g, const double* sh27, const double* moments, const uint8_t* valid,
                                        const mcpt_volume_visibility* v, const double* q6, int64_t n, double* e3, int32_t* corners)
{
    if (const int rc = lookup_check(g, v, sh27, moments, q6, n, e3)) return rc;
    if (n == 0) return MCPT_OK;
    if (const int rc = lookup_arrays_check(*g, *v, sh27, moments, q6, n)) return rc;
    const bool clamp = (g->flags & MCPT_VOLUME_CLAMP_ZERO) != 0;
    for (int64_t r = 0; r < n; r++) {
        int32_t P[8];
        double w[8], AY[MCPT_SH_N];
        const int c = visibility_corners(*g, *v, moments, valid, q6 + r * 6, P, w);
        volume_lobe9(q6 + r * 6 + 3, AY);
        volume_eval(sh27, P, w, AY, c > 0, clamp, e3 + r * 3);
        if (corners) corners[r] = c;
    }
    return MCPT_OK;
}

int mcpt_volume_irradiance_visible_device(mcpt_device* d, const mcpt_volume_grid* g, const double* d_sh27, const double* d_moments, const uint8_t* d_valid,
                                          const mcpt_volume_visibility* v, const double* d_q6, int64_t n, double* d_e3, int32_t* d_corners, void* stream)
{
    if (const int rc = lookup_check(g, v, d_sh27, d_moments, d_q6, n, d_e3)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (n == 0) return MCPT_OK;
    launch_volume_irradiance_visible(*g, *v, d_sh27, d_moments, d_valid, d_q6, n, d_e3, d_corners, static_cast<hipStream_t>(stream));
    return launch_result();
}

int mcpt_volume_irradiance_visible(mcpt_device* d, const mcpt_volume_grid* g, const double* sh27, const double* moments, const uint8_t* valid,
                                   const mcpt_volume_visibility* v, const double* q6, int64_t n, double* e3, int32_t* corners)
{
    if (const int rc = lookup_check(g, v, sh27, moments, q6, n, e3)) return rc;
    if (n > 0)
        if (const int rc = lookup_arrays_check(*g, *v, sh27, moments, q6, n)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (n == 0) return MCPT_OK;
    const size_t probes = size_t(volume_probes(*g)), sn = size_t(n);
    Staging S(d->stream.get());
    const double *d_sh = nullptr, *d_m = nullptr, *d_q = nullptr;
    const uint8_t* d_valid = nullptr;
    double* d_e = nullptr;
    int32_t* d_corners = nullptr;
    if (const int rc = S.in(sh27, probes * MCPT_SH_N * 3, "the volume's coefficients", d_sh)) return rc;
    if (const int rc = S.in(moments, probes * size_t(v->res) * size_t(v->res) * 2, "the volume's moments", d_m)) return rc;
    if (const int rc = S.in(q6, sn * 6, "the receiver list", d_q)) return rc;
    if (const int rc = S.in(valid, probes, "the volume's mask", d_valid)) return rc;
    if (const int rc = S.out(e3, sn * 3, "the receivers' irradiance", d_e)) return rc;
    if (const int rc = S.out(corners, sn, "the receivers' corners", d_corners)) return rc;
    launch_volume_irradiance_visible(*g, *v, d_sh, d_m, d_valid, d_q, n, d_e, d_corners, d->stream.get());
    return S.finish(launch_result());
}

}  // extern "C"
