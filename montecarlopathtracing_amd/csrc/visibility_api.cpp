// C ABI, probe visibility (include/mcpt.h: mcpt_visibility_bin, mcpt_query_visibility*, mcpt_bake_volume_visibility*,
// mcpt_volume_irradiance_visible*): per probe an octahedral map of depth moments and the count of back-face hits, and the irradiance
// volume's lookup weighted by them.  A bake draws the probe query's own rays into a workspace the device keeps (visibility.hip), answers
// them with the unchanged closest-hit launch (kernels.hip: launch_trace_closest_leaf -- mcpt_trace_closest_device's walks, handing back the
// leaf, whose record holds the face normal) and folds chunk by chunk.  The arithmetic is visibility.hpp's, compiled here for the host forms.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>
#include <limits>
#include <string>

#include "handles.hpp"
#include "visibility.hpp"

using namespace mcpt;

static constexpr int64_t kInt32Max = std::numeric_limits<int32_t>::max();
static constexpr int64_t kDefaultWorkspaceRays = int64_t(1) << 22;  // 352 MB of workspace: 64 probes' worth of 65 536 samples, 65 536 probes' of 64
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
    if (n < 0 || n > kInt32Max) return fail(MCPT_ERR_ARG, "the number of probes must be in 0 .. 2^31 - 1");
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
    if (n < 0 || n > kInt32Max) return fail(MCPT_ERR_ARG, "the number of receivers must be in 0 .. 2^31 - 1");
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
    if (!d->vis) {
        auto v = std::make_unique<mcpt_device::Visibility>();
        HIP_TRY(create(v->done, hipEventCreateWithFlags, hipEventDisableTiming));
        d->vis = std::move(v);
    }
    mcpt_device::Visibility& w = *d->vis;
    HIP_TRY(hipEventSynchronize(w.done.get()));             // the bake before this one has left the workspace
    const int64_t budget = vp.workspace_rays > 0 ? vp.workspace_rays : kDefaultWorkspaceRays;
    int64_t per_chunk = budget / vp.spp;                    // whole probes, at least one
    per_chunk = per_chunk < 1 ? 1 : (per_chunk > n ? n : per_chunk);
    const int64_t rays = per_chunk * vp.spp;                // <= 2^62
    if (rays > (int64_t(1) << 40)) return fail(MCPT_ERR_NOMEM, "the visibility workspace of " + std::to_string(rays) + " rays cannot be allocated");
    const size_t sr = size_t(rays);
    if (const int rc = volume_alloc_result(w.rays6.grow_bytes(sr * 6 * sizeof(double)), "the visibility rays", sr * 6 * sizeof(double))) return rc;
    if (const int rc = volume_alloc_result(w.t.grow_bytes(sr * sizeof(double)), "the visibility rays' distances", sr * sizeof(double))) return rc;
    if (const int rc = volume_alloc_result(w.p.grow_bytes(sr * 3 * sizeof(double)), "the visibility rays' hit points", sr * 3 * sizeof(double))) return rc;
    if (const int rc = volume_alloc_result(w.leaf.grow_bytes(sr * sizeof(int32_t)), "the visibility rays' hits", sr * sizeof(int32_t))) return rc;
    static_assert(kRayBytes == 84, "mcpt.h states the workspace's bytes per ray");
    int chunks = 0;
    int rc = MCPT_OK;
    for (int64_t first = 0; first < n && rc == MCPT_OK; first += per_chunk, chunks++) {
        VisChunk c{};
        c.p3 = d_p3; c.ids = d_ids; c.first = first; c.count = n - first < per_chunk ? n - first : per_chunk;
        c.spp = vp.spp; c.sample_base = vp.sample_base; c.seed = vp.seed;
        c.rays6 = w.rays6.get(); c.leaf = w.leaf.get(); c.t = w.t.get();
        launch_visibility_rays(c, st);
        launch_trace_closest_leaf(d->ds, d->trace_mode == MCPT_TRACE_FAST, c.rays6, c.count * c.spp, c.leaf, c.t, w.p.get(), d->aux_ctr.get(), d->aux_queue.get(),
                                  d->aux_slow_list.get(), d->slow_cap, st, d->cfg);
        launch_visibility_fold(d->ds, c, vp, d_moments, d_hits, d_back, d_valid, st);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = fail(MCPT_ERR_HIP, hipGetErrorString(e));
    }
    HIP_TRY(hipEventRecord(w.done.get(), st));              // also after a failure: kernels may be enqueued
    if (rc != MCPT_OK) return rc;
    if (stats) {
        HIP_TRY(hipStreamSynchronize(st));
        stats->rays_primary = stats->samples = uint64_t(n) * uint64_t(vp.spp);
        stats->launches = chunks;
    }
    return MCPT_OK;
}

// what every bake on a device asks before it touches one
static int device_gate(mcpt_device* d)
{
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    HIP_TRY(hipSetDevice(d->ordinal));
    return MCPT_OK;
}

// the grid form on st: the grid's positions into the volume's own list (volume_api.cpp keeps it the same way), then the list form
static int bake_grid_device(mcpt_device* d, const mcpt_volume_grid& g, const mcpt_visibility_params& vp, double* d_moments, int32_t* d_hits, int32_t* d_back,
                            uint8_t* d_valid, mcpt_stats* stats, hipStream_t st)
{
    if (!d->vol) {
        auto v = std::make_unique<mcpt_device::Volume>();
        HIP_TRY(create(v->done, hipEventCreateWithFlags, hipEventDisableTiming));
        d->vol = std::move(v);
    }
    mcpt_device::Volume& v = *d->vol;
    HIP_TRY(hipEventSynchronize(v.done.get()));             // the bake before this one has read its points
    const int64_t n = volume_probes(g);
    const size_t bytes = size_t(n) * 3 * sizeof(double);
    if (const int rc = volume_alloc_result(v.p3.grow_bytes(bytes), "the volume's probe positions", bytes)) return rc;
    launch_volume_points(g, v.p3.get(), st);
    HIP_TRY(hipGetLastError());
    const int rc = bake_device(d, v.p3.get(), nullptr, n, vp, d_moments, d_hits, d_back, d_valid, stats, st);
    HIP_TRY(hipEventRecord(v.done.get(), st));              // also after a failure: k_vol_points is enqueued
    return rc;
}

// A host-pointer bake of n probes: device copies of the answers around run(d_moments, d_hits, d_back, d_valid) on the device's stream
template <class Run>
static int bake_host(mcpt_device* d, int64_t n, int res, double* moments, int32_t* hits, int32_t* back, uint8_t* valid, const Run& run)
{
    const size_t sn = size_t(n), mbytes = sn * size_t(res) * size_t(res) * 2 * sizeof(double);
    DevBuf<double> d_m;
    DevBuf<int32_t> d_hits, d_back;
    DevBuf<uint8_t> d_valid;
    if (const int rc = volume_alloc_result(d_m.alloc_bytes(mbytes), "the probes' moments", mbytes)) return rc;
    if (hits) HIP_TRY(d_hits.alloc(sn));
    if (back) HIP_TRY(d_back.alloc(sn));
    if (valid) HIP_TRY(d_valid.alloc(sn));
    hipStream_t st = d->stream.get();
    int rc = run(d_m.get(), hits ? d_hits.get() : nullptr, back ? d_back.get() : nullptr, valid ? d_valid.get() : nullptr, st);
    const hipError_t e = hipStreamSynchronize(st);          // also on failure: nothing enqueued may still use a copy when it goes
    if (rc == MCPT_OK && e != hipSuccess) rc = fail(MCPT_ERR_HIP, hipGetErrorString(e));
    if (rc != MCPT_OK) return rc;
    HIP_TRY(hipMemcpy(moments, d_m.get(), mbytes, hipMemcpyDeviceToHost));
    if (hits) HIP_TRY(hipMemcpy(hits, d_hits.get(), sn * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (back) HIP_TRY(hipMemcpy(back, d_back.get(), sn * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (valid) HIP_TRY(hipMemcpy(valid, d_valid.get(), sn, hipMemcpyDeviceToHost));
    return MCPT_OK;
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
    const size_t sn = size_t(n);
    DevBuf<double> d_p;
    DevBuf<int32_t> d_ids;
    if (const int rc = volume_alloc_result(d_p.alloc_bytes(sn * 3 * sizeof(double)), "the probe list", sn * 3 * sizeof(double))) return rc;
    if (ids) HIP_TRY(d_ids.alloc(sn));
    HIP_TRY(hipMemcpy(d_p.get(), p3, sn * 3 * sizeof(double), hipMemcpyHostToDevice));
    if (ids) HIP_TRY(hipMemcpy(d_ids.get(), ids, sn * sizeof(int32_t), hipMemcpyHostToDevice));
    return bake_host(d, n, p->res, moments, hits, back, valid, [&](double* m, int32_t* h, int32_t* b, uint8_t* v, hipStream_t st) {
        return bake_device(d, d_p.get(), ids ? d_ids.get() : nullptr, n, *p, m, h, b, v, stats, st);
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
    return bake_host(d, volume_probes(*g), p->res, moments, hits, back, valid, [&](double* m, int32_t* h, int32_t* b, uint8_t* v, hipStream_t st) {
        return bake_grid_device(d, *g, *p, m, h, b, v, stats, st);
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
    HIP_TRY(hipGetLastError());
    return MCPT_OK;
}

int mcpt_volume_irradiance_visible(mcpt_device* d, const mcpt_volume_grid* g, const double* sh27, const double* moments, const uint8_t* valid,
                                   const mcpt_volume_visibility* v, const double* q6, int64_t n, double* e3, int32_t* corners)
{
    if (const int rc = lookup_check(g, v, sh27, moments, q6, n, e3)) return rc;
    if (n > 0)
        if (const int rc = lookup_arrays_check(*g, *v, sh27, moments, q6, n)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (n == 0) return MCPT_OK;
    const size_t probes = size_t(volume_probes(*g)), sn = size_t(n), sh_bytes = probes * MCPT_SH_N * 3 * sizeof(double);
    const size_t m_bytes = probes * size_t(v->res) * size_t(v->res) * 2 * sizeof(double);
    DevBuf<double> d_sh, d_m, d_q, d_e;
    DevBuf<uint8_t> d_valid;
    DevBuf<int32_t> d_corners;
    if (const int rc = volume_alloc_result(d_sh.alloc_bytes(sh_bytes), "the volume's coefficients", sh_bytes)) return rc;
    if (const int rc = volume_alloc_result(d_m.alloc_bytes(m_bytes), "the volume's moments", m_bytes)) return rc;
    if (const int rc = volume_alloc_result(d_q.alloc_bytes(sn * 6 * sizeof(double)), "the receiver list", sn * 6 * sizeof(double))) return rc;
    if (const int rc = volume_alloc_result(d_e.alloc_bytes(sn * 3 * sizeof(double)), "the receivers' irradiance", sn * 3 * sizeof(double))) return rc;
    if (valid) HIP_TRY(d_valid.alloc(probes));
    if (corners) HIP_TRY(d_corners.alloc(sn));
    HIP_TRY(hipMemcpy(d_sh.get(), sh27, sh_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_m.get(), moments, m_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_q.get(), q6, sn * 6 * sizeof(double), hipMemcpyHostToDevice));
    if (valid) HIP_TRY(hipMemcpy(d_valid.get(), valid, probes, hipMemcpyHostToDevice));
    hipStream_t st = d->stream.get();
    launch_volume_irradiance_visible(*g, *v, d_sh.get(), d_m.get(), valid ? d_valid.get() : nullptr, d_q.get(), n, d_e.get(), corners ? d_corners.get() : nullptr, st);
    int rc = MCPT_OK;
    const hipError_t el = hipGetLastError();
    if (el != hipSuccess) rc = fail(MCPT_ERR_HIP, hipGetErrorString(el));
    const hipError_t e = hipStreamSynchronize(st);              // also on failure: nothing enqueued may still use a copy when it goes
    if (rc == MCPT_OK && e != hipSuccess) rc = fail(MCPT_ERR_HIP, hipGetErrorString(e));
    if (rc != MCPT_OK) return rc;
    HIP_TRY(hipMemcpy(e3, d_e.get(), sn * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (corners) HIP_TRY(hipMemcpy(corners, d_corners.get(), sn * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MCPT_OK;
}

}  // extern "C"
