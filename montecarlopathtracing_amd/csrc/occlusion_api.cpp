// C ABI, ambient occlusion (include/mcpt.h: mcpt_query_occlusion*, mcpt_occlusion_fold_host, mcpt_bake_occlusion_lightmap*): per entry of
// a list of surface points the share of its hemisphere that is open, a bent normal and the counts of near and back-face hits.  A query
// draws the irradiance query's own rays into the visibility bake's workspace (occlusion.hip), answers them with the unchanged closest-hit
// launch (hit_work.hpp: trace_leaf) and folds chunk by chunk (chunk_run); a map is that query over the lightmap baker's texel list,
// scattered and dilated on one channel (lightmap_api.cpp: map_bake).  The arithmetic is occlusion.hpp's, compiled here for the host fold.
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
    HitWork& w = *d->vis;
    const int64_t per_chunk = chunk_plan(op.workspace_rays, op.spp, n);     // whole entries
    // (2^38 rays are 256 blocks short of the largest grid of the rays kernel, and 23 TB)
    if (const int rc = hit_work_grow(w, per_chunk * op.spp, int64_t(1) << 38, "occlusion", true)) return rc;
    return chunk_run(n, per_chunk, op.spp, l, stats, st, [&](int64_t first, int64_t count) {
        const OccChunk c{{d_q6, d_ids, first, count, op.spp, op.sample_base, op.seed, w.rays6.get(), w.leaf.get(), w.t.get()}, op.falloff, op.max_distance};
        launch_occlusion_rays(c, st);
        trace_leaf(d, c.rays6, c.count * c.spp, c.leaf, c.t, w.p.get(), st);
        launch_occlusion_fold(d->ds, c, d_ao, d_err, d_bent3, d_hits, d_back, st);
        return launch_result();
    });
}

// The map on st, after the refusals; device pointers throughout: the lightmap baker's spine (lightmap_api.cpp: map_bake) on one channel
// around the query above.  (The map holds d->lm's lease, the query d->vis's.)
static int map_device(mcpt_device* d, const double* d_uv6, const mcpt_occlusion_map& mp, const mcpt_occlusion_params& op, double* d_ao, double* d_err,
                      double* d_bent3, int32_t* d_hits, int32_t* d_back, int32_t* d_owner, mcpt_stats* stats, hipStream_t st)
{
    const size_t n = size_t(mp.width) * mp.height;
    const MapClear clears[] = {{d_err, n * sizeof(double)}, {d_bent3, n * 3 * sizeof(double)}, {d_hits, n * sizeof(int32_t)}, {d_back, n * sizeof(int32_t)}};
    return map_bake(d, d_uv6, mp.width, mp.height, mp.dilate, 1, d_ao, clears, 4, d_owner, stats, st,
                    [&](const int32_t* texels, const double* q6, int32_t covered, double* frame_at) -> int {
        const size_t c = size_t(covered);
        mcpt_device::Lightmap& m = *d->lm;
        if (const int rc = grow(m.occ, c * 5, kWork)) return rc;
        if (const int rc = grow(m.occ_cnt, c * 2, kWork)) return rc;
        // the query's answers by list entry: ao [c], stderr [c], bent [c][3]; hits [c], back [c]
        double *ao = m.occ.get(), *err = d_err ? ao + c : nullptr, *bent = d_bent3 ? ao + 2 * c : nullptr;
        int32_t *hits = d_hits ? m.occ_cnt.get() : nullptr, *back = d_back ? m.occ_cnt.get() + c : nullptr;
        if (const int rc = occlusion_device(d, q6, texels, covered, op, ao, err, bent, hits, back, stats, st)) return rc;
        launch_occlusion_scatter(texels, covered, ao, err, bent, hits, back, frame_at, d_err, d_bent3, d_hits, d_back, st);
        return MCPT_OK;
    });
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
