// C ABI, ambient occlusion (include/mcpt.h: mcpt_query_occlusion*, mcpt_occlusion_fold_host, mcpt_bake_occlusion_lightmap*): per entry of
// a list of surface points the share of its hemisphere that is open, a bent normal and the counts of near and back-face hits.  A query
// draws the irradiance query's own rays into the visibility bake's workspace (occlusion.hip), answers them with the unchanged closest-hit
// launch (kernels.hip: launch_trace_closest_leaf) and folds chunk by chunk; a map is that query over the lightmap baker's texel list
// (lightmap.hip, unchanged), scattered and dilated on one channel.  The arithmetic is occlusion.hpp's, compiled here for the host fold.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>
#include <string>

#include "chunks.hpp"
#include "handles.hpp"
#include "lightmap.hpp"
#include "occlusion.hpp"

using namespace mcpt;

static const char* const kWork = "the lightmap baker's workspace";

// what every call refuses of its parameters, in the struct's field order, then of its count and its two required arrays
static int params_check(const mcpt_occlusion_params* p, int64_t n, const void* q6, const void* ao)
{
    if (!p) return fail(MCPT_ERR_ARG, "null occlusion parameters");
    if (p->spp < 1) return fail(MCPT_ERR_ARG, "spp must be >= 1");
    if (p->sample_base < 0) return fail(MCPT_ERR_ARG, "sample_base must be >= 0");
    if (int64_t(p->sample_base) + int64_t(p->spp) > kInt32Max) return fail(MCPT_ERR_ARG, "sample_base + spp must not exceed 2^31 - 1");
    if (p->falloff != MCPT_OCCLUSION_HARD && p->falloff != MCPT_OCCLUSION_LINEAR && p->falloff != MCPT_OCCLUSION_SQUARE)
        return fail(MCPT_ERR_ARG, "falloff must be MCPT_OCCLUSION_HARD, _LINEAR or _SQUARE");
    if (p->flags != 0) return fail(MCPT_ERR_ARG, "mcpt_occlusion_params.flags must be 0");
    if (!(std::isfinite(p->max_distance) && p->max_distance > 0.0)) return fail(MCPT_ERR_ARG, "max_distance must be finite and > 0");
    if (p->workspace_rays < 0) return fail(MCPT_ERR_ARG, "workspace_rays must be >= 0");
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(MCPT_ERR_ARG, "mcpt_occlusion_params.reserved must be 0");
    if (const int rc = count_check(n, "entries")) return rc;
    if (n > 0 && (!q6 || !ao)) return fail(MCPT_ERR_ARG, "null entry list or occlusion");
    return MCPT_OK;
}

// what both forms of the map refuse: the map's fields in their order, then the parameters, then the one required map
static int map_check(const mcpt_occlusion_map* m, const mcpt_occlusion_params* p, const void* ao)
{
    if (!m) return fail(MCPT_ERR_ARG, "null occlusion map");
    if (const int rc = lightmap_size_check(m->width, m->height)) return rc;
    if (m->dilate < 0 || m->dilate > kLightmapMaxDilate) return fail(MCPT_ERR_ARG, "dilate must be in 0 .. 64");
    if (m->reserved != 0) return fail(MCPT_ERR_ARG, "mcpt_occlusion_map.reserved must be 0");
    if (const int rc = params_check(p, 0, nullptr, nullptr)) return rc;
    if (!ao) return fail(MCPT_ERR_ARG, "null occlusion map array");
    return MCPT_OK;
}

// The query on st, after the refusals; device pointers throughout.  Nothing here waits for st unless the caller asks for statistics.
static int occlusion_device(mcpt_device* d, const double* d_q6, const int32_t* d_ids, int64_t n, const mcpt_occlusion_params& op, double* d_ao,
                            double* d_err, double* d_bent3, int32_t* d_hits, int32_t* d_back, mcpt_stats* stats, hipStream_t st)
{
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return MCPT_OK;
    if (const int rc = motion_home(d)) return rc;           // a device that holds a motion answers from key 0
    if (const int rc = geometry_gate(d)) return rc;
    Lease l;
    if (const int rc = lease(d->vis, st, l)) return rc;     // the visibility or occlusion call before this one has left the workspace
    mcpt_device::Visibility& w = *d->vis;
    const int64_t per_chunk = chunk_plan(op.workspace_rays, op.spp, n);     // whole entries
    const int64_t rays = per_chunk * op.spp;
    // (2^38 rays are 256 blocks short of the largest grid of k_occ_rays, and 23 TB)
    if (rays > (int64_t(1) << 38)) return fail(MCPT_ERR_NOMEM, "the occlusion workspace of " + std::to_string(rays) + " rays cannot be allocated");
    const size_t sr = size_t(rays);
    if (const int rc = grow(w.rays6, sr * 6, "the occlusion rays")) return rc;
    if (const int rc = grow(w.t, sr, "the occlusion rays' distances")) return rc;
    if (const int rc = grow(w.p, sr * 3, "the occlusion rays' hit points")) return rc;
    if (const int rc = grow(w.leaf, sr, "the occlusion rays' hits")) return rc;
    int chunks = 0;
    int rc = MCPT_OK;
    for (int64_t first = 0; first < n && rc == MCPT_OK; first += per_chunk, chunks++) {
        OccChunk c{};
        c.q6 = d_q6; c.ids = d_ids; c.first = first; c.count = chunk_count(per_chunk, n, first);
        c.spp = op.spp; c.sample_base = op.sample_base; c.seed = op.seed; c.falloff = op.falloff; c.max_distance = op.max_distance;
        c.rays6 = w.rays6.get(); c.leaf = w.leaf.get(); c.t = w.t.get();
        launch_occlusion_rays(c, st);
        launch_trace_closest_leaf(d->ds, d->trace_mode == MCPT_TRACE_FAST, c.rays6, c.count * c.spp, c.leaf, c.t, w.p.get(), d->aux_ctr.get(), d->aux_queue.get(),
                                  d->aux_slow_list.get(), d->slow_cap, st, d->cfg);
        launch_occlusion_fold(d->ds, c, d_ao, d_err, d_bent3, d_hits, d_back, st);
        rc = launch_result();
    }
    if ((rc = l.end(rc)) != MCPT_OK) return rc;
    if (stats) {
        HIP_TRY(hipStreamSynchronize(st));
        stats->rays_primary = stats->samples = uint64_t(n) * uint64_t(op.spp);
        stats->launches = chunks;
    }
    return MCPT_OK;
}

// The map on st, after the refusals; device pointers throughout.  The host waits once, for the number of covered texels.
static int map_device(mcpt_device* d, const double* d_uv6, const mcpt_occlusion_map& mp, const mcpt_occlusion_params& op, double* d_ao, double* d_err,
                      double* d_bent3, int32_t* d_hits, int32_t* d_back, int32_t* d_owner, mcpt_stats* stats, hipStream_t st)
{
    if (const int rc = lightmap_device_gate(d)) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    const int W = mp.width, H = mp.height, R = mp.dilate;
    const size_t n = size_t(W) * H;
    LightmapWork w{};
    Lease l;                                                // (d->lm's: the query below holds d->vis's)
    if (const int rc = lightmap_ensure_work(d, W, H, w, st, l)) return rc;
    mcpt_device::Lightmap& m = *d->lm;
    if (R > 0) {
        if (const int rc = grow(m.owner[1], n, kWork)) return rc;
        if (const int rc = grow(m.irr, n, kWork)) return rc;
    }
    // the lightmap's raster (lightmap.hip) and the covered count, which the host waits for: 4 bytes back
    launch_lightmap_raster(d->ds, d_uv6, W, H, w, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(m.h_total.get(), w.total, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int32_t covered = m.h_total[0];
    // the rounds alternate between the caller's frame and the baker's own: the scatter starts where R rounds end in the caller's
    double* frame[2] = {d_ao, m.irr.get()};
    int at = R & 1;
    HIP_TRY(hipMemsetAsync(frame[at], 0, n * sizeof(double), st));
    if (d_err) HIP_TRY(hipMemsetAsync(d_err, 0, n * sizeof(double), st));
    if (d_bent3) HIP_TRY(hipMemsetAsync(d_bent3, 0, n * 3 * sizeof(double), st));
    if (d_hits) HIP_TRY(hipMemsetAsync(d_hits, 0, n * sizeof(int32_t), st));
    if (d_back) HIP_TRY(hipMemsetAsync(d_back, 0, n * sizeof(int32_t), st));
    if (covered > 0) {
        const size_t c = size_t(covered);
        if (const int rc = grow(m.texels, c, kWork)) return rc;
        if (const int rc = grow(m.q6, c * 6, kWork)) return rc;
        if (const int rc = grow(m.occ, c * 5, kWork)) return rc;
        if (const int rc = grow(m.occ_cnt, c * 2, kWork)) return rc;
        launch_lightmap_texels(d->ds, d_uv6, W, H, w, m.texels.get(), m.q6.get(), st);
        HIP_TRY(hipGetLastError());
        // the query's answers by list entry: ao [c], stderr [c], bent [c][3]; hits [c], back [c]
        double *ao = m.occ.get(), *err = d_err ? ao + c : nullptr, *bent = d_bent3 ? ao + 2 * c : nullptr;
        int32_t *hits = d_hits ? m.occ_cnt.get() : nullptr, *back = d_back ? m.occ_cnt.get() + c : nullptr;
        if (const int rc = occlusion_device(d, m.q6.get(), m.texels.get(), covered, op, ao, err, bent, hits, back, stats, st)) return rc;
        launch_occlusion_scatter(m.texels.get(), covered, ao, err, bent, hits, back, frame[at], d_err, d_bent3, d_hits, d_back, st);
        HIP_TRY(hipGetLastError());
    }
    int32_t* own[2] = {m.owner[0].get(), m.owner[1].get()};
    for (int r = 1; r <= R; r++) {
        launch_occlusion_dilate(frame[at], own[(r - 1) & 1], W, H, r, frame[at ^ 1], own[r & 1], st);
        at ^= 1;
    }
    HIP_TRY(hipGetLastError());
    if (d_owner) HIP_TRY(hipMemcpyAsync(d_owner, own[R & 1], n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return l.end(MCPT_OK);
}

extern "C" {

int mcpt_occlusion_fold_host(const double* q6, const double* rays6, const int32_t* hit, const double* t, const double* n3, int64_t n,
                             const mcpt_occlusion_params* p, double* ao, double* stderr1, double* bent3, int32_t* hits, int32_t* back)
{
    if (const int rc = params_check(p, n, q6, ao)) return rc;
    if (n > 0 && (!rays6 || !hit || !t || !n3)) return fail(MCPT_ERR_ARG, "null rays, hit flags, distances or normals");
    for (int64_t i = 0; i < n; i++) {
        OccSums a;
        occlusion_clear(a);
        for (int64_t k = i * p->spp; k < (i + 1) * p->spp; k++)
            occlusion_add(a, occlusion_sample(p->falloff, p->max_distance, rays6 + k * 6 + 3, hit[k] != 0, t[k], n3 + k * 3));
        ao[i] = a.s1 / p->spp;
        if (stderr1) stderr1[i] = occlusion_stderr(a.s1, a.s2, p->spp);
        if (bent3) occlusion_bent(a.b, q6 + i * 6 + 3, bent3 + i * 3);
        if (hits) hits[i] = a.hits;
        if (back) back[i] = a.back;
    }
    return MCPT_OK;
}

int mcpt_query_occlusion_device(mcpt_device* d, const double* d_q6, const int32_t* d_ids, int64_t n, const mcpt_occlusion_params* p, double* d_ao,
                                double* d_stderr1, double* d_bent3, int32_t* d_hits, int32_t* d_back, mcpt_stats* stats, void* stream)
{
    if (const int rc = params_check(p, n, d_q6, d_ao)) return rc;
    if (const int rc = device_gate(d)) return rc;
    return occlusion_device(d, d_q6, d_ids, n, *p, d_ao, d_stderr1, d_bent3, d_hits, d_back, stats, static_cast<hipStream_t>(stream));
}

int mcpt_query_occlusion(mcpt_device* d, const double* q6, const int32_t* ids, int64_t n, const mcpt_occlusion_params* p, double* ao, double* stderr1,
                         double* bent3, int32_t* hits, int32_t* back, mcpt_stats* stats)
{
    if (const int rc = params_check(p, n, q6, ao)) return rc;
    if (const int rc = query_list_check(q6, ids, n, MCPT_QUERY_HEMISPHERE)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return MCPT_OK;
    const size_t sn = size_t(n);
    Staging S(d->stream.get());
    const double* d_q = nullptr;
    const int32_t* d_ids = nullptr;
    double *d_ao = nullptr, *d_err = nullptr, *d_bent = nullptr;
    int32_t *d_hits = nullptr, *d_back = nullptr;
    if (const int rc = S.in(q6, sn * 6, "the entry list", d_q)) return rc;
    if (const int rc = S.in(ids, sn, "the entries' ids", d_ids)) return rc;
    if (const int rc = S.out(ao, sn, "the entries' occlusion", d_ao)) return rc;
    if (const int rc = S.out(stderr1, sn, "the entries' standard error", d_err)) return rc;
    if (const int rc = S.out(bent3, sn * 3, "the entries' bent normals", d_bent)) return rc;
    if (const int rc = S.out(hits, sn, "the entries' hits", d_hits)) return rc;
    if (const int rc = S.out(back, sn, "the entries' back-face hits", d_back)) return rc;
    return S.finish(occlusion_device(d, d_q, d_ids, n, *p, d_ao, d_err, d_bent, d_hits, d_back, stats, d->stream.get()));
}

int mcpt_bake_occlusion_lightmap_device(mcpt_device* d, const double* d_uv6, const mcpt_occlusion_map* m, const mcpt_occlusion_params* p, double* d_ao,
                                        double* d_stderr1, double* d_bent3, int32_t* d_hits, int32_t* d_back, int32_t* d_owner, mcpt_stats* stats,
                                        void* stream)
{
    if (const int rc = map_check(m, p, d_ao)) return rc;
    return map_device(d, d_uv6, *m, *p, d_ao, d_stderr1, d_bent3, d_hits, d_back, d_owner, stats, static_cast<hipStream_t>(stream));
}

int mcpt_bake_occlusion_lightmap(mcpt_device* d, const double* uv6, const mcpt_occlusion_map* m, const mcpt_occlusion_params* p, double* ao,
                                 double* stderr1, double* bent3, int32_t* hits, int32_t* back, int32_t* owner, mcpt_stats* stats)
{
    if (const int rc = map_check(m, p, ao)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (uv6)
        if (const int rc = lightmap_chart_check(uv6, d->ds.t)) return rc;
    const size_t n = size_t(m->width) * m->height;
    Staging S(d->stream.get());
    const double* d_uv = nullptr;                           // (null stays null: the scene's own vt)
    double *d_ao = nullptr, *d_err = nullptr, *d_bent = nullptr;
    int32_t *d_hits = nullptr, *d_back = nullptr, *d_owner = nullptr;
    if (const int rc = S.in(uv6, size_t(d->ds.t) * 6, "the chart", d_uv)) return rc;
    if (const int rc = S.out(ao, n, "the occlusion map", d_ao)) return rc;
    if (const int rc = S.out(stderr1, n, "the standard error map", d_err)) return rc;
    if (const int rc = S.out(bent3, n * 3, "the bent normal map", d_bent)) return rc;
    if (const int rc = S.out(hits, n, "the hit map", d_hits)) return rc;
    if (const int rc = S.out(back, n, "the back-face hit map", d_back)) return rc;
    if (const int rc = S.out(owner, n, "the owner map", d_owner)) return rc;
    return S.finish(map_device(d, d_uv, *m, *p, d_ao, d_err, d_bent, d_hits, d_back, d_owner, stats, d->stream.get()));
}

}  // extern "C"
