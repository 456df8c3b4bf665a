// C ABI, direct light from a caller's own lights (include/mcpt.h: mcpt_query_direct*, mcpt_direct_slots, mcpt_direct_rays,
// mcpt_direct_fold_host, mcpt_bake_direct_lightmap*): per entry of a list of surface points the irradiance that point, spot, directional
// and rectangle lights send there past the scene's geometry, answered by one fused kernel (direct.hip) that forms every shadow ray in
// registers and walks it with the any-hit walk; a map is that query over the lightmap baker's texel list, scattered and dilated on three
// channels (lightmap_api.cpp: map_bake).  The arithmetic is direct.hpp's, compiled here for the light table and the host fold.  The
// device keeps the table of a call in a pinned and a device copy of its own (mcpt_device::Direct) under staging.hpp's lease: a _device
// call returns with its kernels enqueued, and the caller's lights are read before it returns.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>
#include <string>

#include "direct.hpp"
#include "handles.hpp"
#include "lightmap.hpp"

using namespace mcpt;

static const char* const kWork = "the lightmap baker's workspace";
static const char* const kTable = "the light table";

static bool finite3(const double* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }
static bool length_ok(const double* v)
{
    const double l = direct_len(v);
    return l > 0.0 && std::isfinite(l);
}

// what every call refuses of its parameters, in the struct's field order
static int params_check(const mcpt_direct_params* p)
{
    if (!p) return fail(MCPT_ERR_ARG, "null direct parameters");
    if (p->spp < 1) return fail(MCPT_ERR_ARG, "spp must be >= 1");
    if (p->sample_base < 0) return fail(MCPT_ERR_ARG, "sample_base must be >= 0");
    if (int64_t(p->sample_base) + int64_t(p->spp) > kInt32Max) return fail(MCPT_ERR_ARG, "sample_base + spp must not exceed 2^31 - 1");
    if (!(std::isfinite(p->bias) && p->bias >= 0.0)) return fail(MCPT_ERR_ARG, "bias must be finite and >= 0");
    if (p->flags != 0) return fail(MCPT_ERR_ARG, "mcpt_direct_params.flags must be 0");
    if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0) return fail(MCPT_ERR_ARG, "mcpt_direct_params.reserved must be 0");
    return MCPT_OK;
}

// what every call refuses of its lights: the count, the array, then light by light, per light in the header's order, looking only at
// the fields its type reads
static int lights_check(const mcpt_direct_light* lights, int32_t nl)
{
    if (nl < 0 || nl > kDirectMaxLights) return fail(MCPT_ERR_ARG, "the number of lights must be in 0 .. 4096");
    if (nl > 0 && !lights) return fail(MCPT_ERR_ARG, "null lights");
    for (int32_t i = 0; i < nl; i++) {
        const mcpt_direct_light& L = lights[i];
        const std::string who = "light " + std::to_string(i) + ": ";
        const bool point = L.type == MCPT_LIGHT_POINT, spot = L.type == MCPT_LIGHT_SPOT, dir = L.type == MCPT_LIGHT_DIRECTIONAL, rect = L.type == MCPT_LIGHT_RECT;
        if (!point && !spot && !dir && !rect) return fail(MCPT_ERR_ARG, who + "unknown type");
        if ((L.flags & ~MCPT_LIGHT_TWO_SIDED) != 0 || (L.flags != 0 && !rect)) return fail(MCPT_ERR_ARG, who + "flags must be 0, or MCPT_LIGHT_TWO_SIDED on a rectangle");
        bool fin = finite3(L.color);
        if (!dir) fin = fin && finite3(L.position);
        if (spot || dir) fin = fin && finite3(L.direction);
        if (rect) fin = fin && finite3(L.u) && finite3(L.v);
        if (spot) fin = fin && std::isfinite(L.cos_inner) && std::isfinite(L.cos_outer);
        if (point || spot) fin = fin && std::isfinite(L.range);
        if (!fin) return fail(MCPT_ERR_ARG, who + "a component is not finite");
        if ((spot || dir) && !length_ok(L.direction)) return fail(MCPT_ERR_ARG, who + "direction must have a finite length > 0");
        if (rect) {
            double N[3];
            direct_cross(L.u, L.v, N);
            if (!length_ok(N)) return fail(MCPT_ERR_ARG, who + "cross(u, v) must have a finite length > 0");
        }
        if (spot && !(-1.0 <= L.cos_outer && L.cos_outer < L.cos_inner && L.cos_inner <= 1.0))
            return fail(MCPT_ERR_ARG, who + "the cosines must satisfy -1 <= cos_outer < cos_inner <= 1");
        if ((point || spot) && L.range < 0.0) return fail(MCPT_ERR_ARG, who + "range must be >= 0");
    }
    return MCPT_OK;
}

// R of checked lights: at most 4096 * (2^31 - 1)
static int64_t slots_of(const mcpt_direct_light* lights, int32_t nl, int32_t spp)
{
    int64_t R = 0;
    for (int32_t i = 0; i < nl; i++) R += direct_light_slots(lights[i].type, spp);
    return R;
}

static int slots_bound_check(int64_t n, int64_t R)
{
    // (n <= 2^31 - 1 and R <= 2^43: the product stays below 2^63 only while R does not pass the bound itself)
    if (n > 0 && (R > kDirectSlotMax || n * R > kDirectSlotMax)) return fail(MCPT_ERR_ARG, "n * R must not exceed 2^31 - 1 slots");
    return MCPT_OK;
}

// the refusals every call shares, in the header's order: the parameters, the lights, the count, the n * R bound
static int call_check(const mcpt_direct_params* p, const mcpt_direct_light* lights, int32_t nl, int64_t n)
{
    if (const int rc = params_check(p)) return rc;
    if (const int rc = lights_check(lights, nl)) return rc;
    if (const int rc = count_check(n, "entries")) return rc;
    return slots_bound_check(n, slots_of(lights, nl, p->spp));
}

// what both forms of the map refuse: the map's fields in their order, then the parameters and the lights, then the one required map
static int map_check(const mcpt_direct_map* m, const mcpt_direct_params* p, const mcpt_direct_light* lights, int32_t nl, const void* irr)
{
    if (!m) return fail(MCPT_ERR_ARG, "null direct map");
    if (const int rc = lightmap_size_check(m->width, m->height)) return rc;
    if (m->dilate < 0 || m->dilate > kLightmapMaxDilate) return fail(MCPT_ERR_ARG, "dilate must be in 0 .. 64");
    if (m->reserved != 0) return fail(MCPT_ERR_ARG, "mcpt_direct_map.reserved must be 0");
    if (const int rc = call_check(p, lights, nl, 0)) return rc;
    if (!irr) return fail(MCPT_ERR_ARG, "null irradiance map");
    return MCPT_OK;
}

static bool fast_walk(const mcpt_device* d) { return d->trace_mode == MCPT_TRACE_FAST && d->ds.fast.enabled != 0; }

// The table of a call in the device's own copies, on st, under the lease l (which waits for the call before this one to have left them);
// the caller's lights are not read after this returns.
static int table_upload(mcpt_device* d, const mcpt_direct_light* lights, int32_t nl, hipStream_t st, Lease& l, const DirectLight*& d_table)
{
    if (const int rc = lease(d->direct, st, l)) return rc;
    mcpt_device::Direct& w = *d->direct;
    d_table = nullptr;
    if (nl == 0) return MCPT_OK;
    const size_t bytes = size_t(nl) * sizeof(DirectLight);
    if (const int rc = alloc_result(w.h_lights.grow_bytes(bytes), kTable, bytes)) return rc;
    if (const int rc = alloc_result(w.lights.grow_bytes(bytes), kTable, bytes)) return rc;
    DirectLight* h = reinterpret_cast<DirectLight*>(w.h_lights.get());
    for (int32_t i = 0; i < nl; i++) h[i] = direct_prepare(lights[i]);
    HIP_TRY(hipMemcpyAsync(w.lights.get(), h, bytes, hipMemcpyHostToDevice, st));
    d_table = reinterpret_cast<const DirectLight*>(w.lights.get());
    return MCPT_OK;
}

static DirectCall call_of(const double* d_q6, const int32_t* d_ids, int64_t n, const DirectLight* table, int32_t nl, const mcpt_direct_params& p)
{
    return DirectCall{d_q6, d_ids, n, table, nl, p.spp, p.sample_base, p.seed, p.bias};
}

// The query on st, after the refusals and the device gate; device pointers throughout but for the lights.  Nothing here waits for st
// unless the caller asks for statistics: then the counters are cleared before the launch and read after it, between two events.
static int direct_device(mcpt_device* d, const double* d_q6, const int32_t* d_ids, int64_t n, const mcpt_direct_light* lights, int32_t nl,
                         const mcpt_direct_params& p, double* d_irr, double* d_err, double* d_pl, double* d_vis, mcpt_stats* stats, hipStream_t st)
{
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (const int rc = motion_home(d)) return rc;           // a device that holds a motion answers from key 0
    if (const int rc = geometry_gate(d)) return rc;
    if (n == 0) return MCPT_OK;
    if (const int rc = slots_bound_check(n, slots_of(lights, nl, p.spp))) return rc;    // (a map learns its n here)
    Lease l;
    const DirectLight* table = nullptr;
    if (const int rc = table_upload(d, lights, nl, st, l, table)) return rc;
    if (stats) {
        HIP_TRY(hipMemsetAsync(d->aux_ctr.get(), 0, sizeof(DCounters), st));
        HIP_TRY(hipEventRecord(d->ev[0].get(), st));
    }
    launch_direct(d->ds, fast_walk(d), call_of(d_q6, d_ids, n, table, nl, p), d_irr, d_err, d_pl, d_vis, d->aux_ctr.get(), d->cfg.cus, st);
    int rc = launch_result();
    if (rc == MCPT_OK && stats) {
        const hipError_t e = hipEventRecord(d->ev[1].get(), st);
        if (e != hipSuccess) rc = fail(MCPT_ERR_HIP, std::string("hipEventRecord: ") + hipGetErrorString(e));
    }
    if (const int rc2 = l.end(rc)) return rc2;
    if (!stats) return MCPT_OK;
    HIP_TRY(hipStreamSynchronize(st));
    DCounters c{};
    HIP_TRY(hipMemcpy(&c, d->aux_ctr.get(), sizeof c, hipMemcpyDeviceToHost));
    counters_to_stats(c, stats, d->knobs.print_diag != 0);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, d->ev[0].get(), d->ev[1].get());
    stats->ms_trace = ms; stats->ms_total = ms; stats->launches = 1;
    return MCPT_OK;
}

// The map on st, after the refusals; device pointers throughout but for the lights: the lightmap baker's spine on three channels around
// the query above.  (The map holds d->lm's lease, the query d->direct's.)
static int map_device(mcpt_device* d, const double* d_uv6, const mcpt_direct_map& mp, const mcpt_direct_light* lights, int32_t nl, const mcpt_direct_params& p,
                      double* d_irr, double* d_err, double* d_pl, double* d_vis, int32_t* d_owner, mcpt_stats* stats, hipStream_t st)
{
    const size_t n = size_t(mp.width) * mp.height, snl = size_t(nl);
    const MapClear clears[] = {{d_err, n * 3 * sizeof(double)}, {nl ? d_pl : nullptr, n * snl * 3 * sizeof(double)}, {nl ? d_vis : nullptr, n * snl * sizeof(double)}};
    return map_bake(d, d_uv6, mp.width, mp.height, mp.dilate, 3, d_irr, clears, 3, d_owner, stats, st,
                    [&](const int32_t* texels, const double* q6, int32_t covered, double* frame_at) -> int {
        const size_t c = size_t(covered);
        mcpt_device::Lightmap& m = *d->lm;
        // the query's answers by list entry: irradiance [c][3], stderr [c][3], per light [c][nl][3], visibility [c][nl]
        if (const int rc = grow(m.direct, c * (6 + 4 * snl), kWork)) return rc;
        double *irr = m.direct.get(), *err = d_err ? irr + c * 3 : nullptr, *pl = d_pl ? irr + c * 6 : nullptr, *vis = d_vis ? irr + c * (6 + 3 * snl) : nullptr;
        if (const int rc = direct_device(d, q6, texels, covered, lights, nl, p, irr, err, pl, vis, stats, st)) return rc;
        launch_direct_scatter(texels, covered, 3, irr, frame_at, st);
        launch_direct_scatter(texels, covered, 3, err, d_err, st);
        launch_direct_scatter(texels, covered, nl * 3, pl, d_pl, st);
        launch_direct_scatter(texels, covered, nl, vis, d_vis, st);
        return MCPT_OK;
    });
}

extern "C" {

int64_t mcpt_direct_slots(const mcpt_direct_light* lights, int32_t nl, int32_t spp)
{
    if (spp < 1) return fail(MCPT_ERR_ARG, "spp must be >= 1");
    if (const int rc = lights_check(lights, nl)) return rc;
    return slots_of(lights, nl, spp);
}

int mcpt_direct_fold_host(const mcpt_direct_light* lights, int32_t nl, const mcpt_direct_params* p, const double* g, const uint8_t* occluded, int64_t n,
                          double* irradiance3, double* stderr3, double* per_light3, double* visibility)
{
    if (const int rc = call_check(p, lights, nl, n)) return rc;
    const int64_t R = slots_of(lights, nl, p->spp);
    if (n > 0 && (!irradiance3 || (R > 0 && (!g || !occluded)))) return fail(MCPT_ERR_ARG, "null g, occluded or irradiance");
    for (int64_t i = 0; i < n; i++) {
        DirectFold f;
        f.begin();
        int64_t at = i * R;
        for (int32_t l = 0; l < nl; l++) {
            const DirectLight D = direct_prepare(lights[l]);
            const int32_t slots = direct_light_slots(D.type, p->spp);
            f.light_begin();
            for (int32_t j = 0; j < slots; j++, at++) f.add(D, g[at], occluded[at] != 0);
            f.light_end(D, p->spp);
            if (per_light3)
                for (int c = 0; c < 3; c++) per_light3[(i * nl + l) * 3 + c] = f.El[c];
            if (visibility) visibility[i * nl + l] = f.vis;
        }
        for (int c = 0; c < 3; c++) {
            irradiance3[i * 3 + c] = f.E[c];
            if (stderr3) stderr3[i * 3 + c] = std::sqrt(f.V[c]);
        }
    }
    return MCPT_OK;
}

int mcpt_query_direct_device(mcpt_device* d, const double* dev_q6, const int32_t* dev_ids, int64_t n, const mcpt_direct_light* lights, int32_t nl,
                             const mcpt_direct_params* p, double* dev_irradiance3, double* dev_stderr3, double* dev_per_light3, double* dev_visibility,
                             void* stream)
{
    if (const int rc = call_check(p, lights, nl, n)) return rc;
    if (n > 0 && (!dev_q6 || !dev_irradiance3)) return fail(MCPT_ERR_ARG, "null entry list or irradiance");
    if (const int rc = device_gate(d)) return rc;
    return direct_device(d, dev_q6, dev_ids, n, lights, nl, *p, dev_irradiance3, dev_stderr3, dev_per_light3, dev_visibility, nullptr,
                         static_cast<hipStream_t>(stream));
}

int mcpt_query_direct(mcpt_device* d, const double* q6, const int32_t* ids, int64_t n, const mcpt_direct_light* lights, int32_t nl,
                      const mcpt_direct_params* p, double* irradiance3, double* stderr3, double* per_light3, double* visibility, mcpt_stats* stats)
{
    if (const int rc = call_check(p, lights, nl, n)) return rc;
    if (n > 0 && (!q6 || !irradiance3)) return fail(MCPT_ERR_ARG, "null entry list or irradiance");
    if (const int rc = query_list_check(q6, ids, n, MCPT_QUERY_HEMISPHERE)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return MCPT_OK;
    const size_t sn = size_t(n), snl = size_t(nl);
    Staging S(d->stream.get());
    const double* d_q = nullptr;
    const int32_t* d_ids = nullptr;
    double *d_irr = nullptr, *d_err = nullptr, *d_pl = nullptr, *d_vis = nullptr;
    if (const int rc = S.in(q6, sn * 6, "the entry list", d_q)) return rc;
    if (const int rc = S.in(ids, sn, "the entries' ids", d_ids)) return rc;
    if (const int rc = S.out(irradiance3, sn * 3, "the entries' irradiance", d_irr)) return rc;
    if (const int rc = S.out(stderr3, sn * 3, "the entries' standard error", d_err)) return rc;
    if (const int rc = S.out(per_light3, sn * snl * 3, "the entries' irradiance by light", d_pl)) return rc;
    if (const int rc = S.out(visibility, sn * snl, "the entries' visibility by light", d_vis)) return rc;
    return S.finish(direct_device(d, d_q, d_ids, n, lights, nl, *p, d_irr, d_err, d_pl, d_vis, stats, d->stream.get()));
}

int mcpt_direct_rays(mcpt_device* d, const double* q6, const int32_t* ids, int64_t n, const mcpt_direct_light* lights, int32_t nl,
                     const mcpt_direct_params* p, double* rays6, double* tmax, double* g)
{
    if (const int rc = call_check(p, lights, nl, n)) return rc;
    const int64_t R = slots_of(lights, nl, p->spp);
    if (n > 0 && (!q6 || (R > 0 && (!rays6 || !tmax || !g)))) return fail(MCPT_ERR_ARG, "null entry list, rays6, tmax or g");
    if (const int rc = query_list_check(q6, ids, n, MCPT_QUERY_HEMISPHERE)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (n == 0 || R == 0) return MCPT_OK;
    const size_t sn = size_t(n), slots = size_t(n * R);
    hipStream_t st = d->stream.get();
    Staging S(st);
    const double* d_q = nullptr;
    const int32_t* d_ids = nullptr;
    double *d_rays = nullptr, *d_tmax = nullptr, *d_g = nullptr;
    if (const int rc = S.in(q6, sn * 6, "the entry list", d_q)) return rc;
    if (const int rc = S.in(ids, sn, "the entries' ids", d_ids)) return rc;
    if (const int rc = S.out(rays6, slots * 6, "the slots' rays", d_rays)) return rc;
    if (const int rc = S.out(tmax, slots, "the slots' limits", d_tmax)) return rc;
    if (const int rc = S.out(g, slots, "the slots' factors", d_g)) return rc;
    Lease l;
    const DirectLight* table = nullptr;
    int rc = table_upload(d, lights, nl, st, l, table);
    if (rc == MCPT_OK) {
        launch_direct_rays(call_of(d_q, d_ids, n, table, nl, *p), R, d_rays, d_tmax, d_g, st);
        rc = l.end(launch_result());
    }
    return S.finish(rc);
}

int mcpt_bake_direct_lightmap_device(mcpt_device* d, const double* dev_uv6, const mcpt_direct_map* m, const mcpt_direct_light* lights, int32_t nl,
                                     const mcpt_direct_params* p, double* dev_irradiance3, double* dev_stderr3, double* dev_per_light3,
                                     double* dev_visibility, int32_t* dev_owner, mcpt_stats* stats, void* stream)
{
    if (const int rc = map_check(m, p, lights, nl, dev_irradiance3)) return rc;
    return map_device(d, dev_uv6, *m, lights, nl, *p, dev_irradiance3, dev_stderr3, dev_per_light3, dev_visibility, dev_owner, stats,
                      static_cast<hipStream_t>(stream));
}

int mcpt_bake_direct_lightmap(mcpt_device* d, const double* uv6, const mcpt_direct_map* m, const mcpt_direct_light* lights, int32_t nl,
                              const mcpt_direct_params* p, double* irradiance3, double* stderr3, double* per_light3, double* visibility, int32_t* owner,
                              mcpt_stats* stats)
{
    if (const int rc = map_check(m, p, lights, nl, irradiance3)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (uv6)
        if (const int rc = lightmap_chart_check(uv6, d->ds.t)) return rc;
    const size_t n = size_t(m->width) * m->height, snl = size_t(nl);
    Staging S(d->stream.get());
    const double* d_uv = nullptr;                           // (null stays null: the scene's own vt)
    double *d_irr = nullptr, *d_err = nullptr, *d_pl = nullptr, *d_vis = nullptr;
    int32_t* d_owner = nullptr;
    if (const int rc = S.in(uv6, size_t(d->ds.t) * 6, "the chart", d_uv)) return rc;
    if (const int rc = S.out(irradiance3, n * 3, "the irradiance map", d_irr)) return rc;
    if (const int rc = S.out(stderr3, n * 3, "the standard error map", d_err)) return rc;
    if (const int rc = S.out(per_light3, n * snl * 3, "the irradiance map by light", d_pl)) return rc;
    if (const int rc = S.out(visibility, n * snl, "the visibility map by light", d_vis)) return rc;
    if (const int rc = S.out(owner, n, "the owner map", d_owner)) return rc;
    return S.finish(map_device(d, d_uv, *m, lights, nl, *p, d_irr, d_err, d_pl, d_vis, d_owner, stats, d->stream.get()));
}

}  // extern "C"
