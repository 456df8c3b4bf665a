// C ABI, lightmap baking (include/mcpt.h: mcpt_lightmap_*, mcpt_bake_lightmap*): a UV chart is rasterised into a map of texels, the
// covered texels become a list of surface points, mcpt_query_radiance's hemisphere kind answers that list (query_api.cpp: query_device,
// unchanged), and the answers go back into the map, whose gutters are dilated.  Everything but the host rasteriser runs on the GPU
// (lightmap.hip); the host waits once per call, for the number of covered texels.  The spine of a bake (map_bake) is the occlusion
// map's as well (occlusion_api.cpp), and the dilation's round loop (lightmap_dilate_rounds) the denoiser's.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>
#include <string>

#include "handles.hpp"
#include "lightmap.hpp"

using namespace mcpt;

static const char* const kWork = "the lightmap baker's workspace";

int lightmap_size_check(int32_t width, int32_t height)
{
    return width >= 1 && width <= kLightmapMaxSize && height >= 1 && height <= kLightmapMaxSize
               ? MCPT_OK
               : fail(MCPT_ERR_ARG, "a lightmap's width and height must be in 1 .. 16384");
}

int lightmap_chart_check(const double* uv6, int64_t num_faces)
{
    for (int64_t i = 0; i < num_faces * 6; i++)
        if (!std::isfinite(uv6[i])) return fail(MCPT_ERR_ARG, "chart of face " + std::to_string(i / 6) + ": component that is not finite");
    return MCPT_OK;
}

// what both forms of mcpt_bake_lightmap refuse without looking at the chart
static int params_check(const mcpt_lightmap_params* p, const void* irradiance3)
{
    if (!p) return fail(MCPT_ERR_ARG, "null lightmap parameters");
    if (const int rc = lightmap_size_check(p->width, p->height)) return rc;
    if (const int rc = range_check(p->spp, p->sample_base, int64_t(p->width) * p->height)) return rc;
    if (const int rc = flags_check(p->flags)) return rc;
    if (p->dilate < 0 || p->dilate > kLightmapMaxDilate) return fail(MCPT_ERR_ARG, "dilate must be in 0 .. 64");
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(MCPT_ERR_ARG, "mcpt_lightmap_params.reserved must be 0");
    if (!irradiance3) return fail(MCPT_ERR_ARG, "null irradiance map");
    return MCPT_OK;
}

// what every call on a device does before it reads the device's triangles: the device itself, key 0 of a motion, a geometry that stands
int lightmap_device_gate(mcpt_device* d)
{
    if (const int rc = device_gate(d)) return rc;
    if (const int rc = motion_home(d)) return rc;
    return geometry_gate(d);
}

// the workspace of a W x H map on d for a call on st, once the bake or denoise before this one has left it
int lightmap_ensure_work(mcpt_device* d, int W, int H, LightmapWork& w, hipStream_t st, Lease& l)
{
    const auto words = [](mcpt_device::Lightmap& m) -> int {
        HIP_TRY(m.h_total.alloc(1));
        HIP_TRY(m.total.alloc(1));
        HIP_TRY(m.n_big.alloc(1));
        return MCPT_OK;
    };
    if (const int rc = lease(d->lm, st, l, words)) return rc;
    mcpt_device::Lightmap& m = *d->lm;
    const size_t n = size_t(W) * H, t = size_t(d->ds.t > 0 ? d->ds.t : 1), blocks = size_t(lightmap_blocks((long long)n));
    if (const int rc = grow(m.owner[0], n, kWork)) return rc;
    if (const int rc = grow(m.slot_of_face, t, kWork)) return rc;
    if (const int rc = grow(m.big, t, kWork)) return rc;
    if (const int rc = grow(m.masks, blocks * 4, kWork)) return rc;
    if (const int rc = grow(m.block_counts, blocks, kWork)) return rc;
    if (const int rc = grow(m.block_offsets, blocks, kWork)) return rc;
    w = LightmapWork{m.owner[0].get(), m.slot_of_face.get(), m.big.get(), m.n_big.get(), m.masks.get(), m.block_counts.get(), m.block_offsets.get(),
                     m.total.get()};
    return MCPT_OK;
}

// Step 1 on st and the number of covered texels, which the host waits for: 4 bytes back.
int lightmap_raster_device(mcpt_device* d, const double* d_uv6, int W, int H, const LightmapWork& w, hipStream_t st, int32_t& covered)
{
    launch_lightmap_raster(d->ds, d_uv6, W, H, w, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(d->lm->h_total.get(), w.total, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    covered = d->lm->h_total[0];
    return MCPT_OK;
}

// Step 5, rounds 1 .. R: the one loop of the two bakes, the occlusion map and the denoiser.
void lightmap_dilate_rounds(double* const frame[2], int32_t* const own[2], int W, int H, int R, int channels, int& at, hipStream_t st)
{
    for (int r = 1; r <= R; r++) {
        launch_lightmap_dilate(frame[at], own[(r - 1) & 1], W, H, r, frame[at ^ 1], own[r & 1], channels, st);
        at ^= 1;
    }
}

// Steps 1 to 5 on st, after the refusals; device pointers throughout.  Step 3, the answers to the texel list, and step 4, their scatter
// into frame_at, are the caller's `answer`.
int map_bake(mcpt_device* d, const double* d_uv6, int W, int H, int R, int channels, double* d_map, const MapClear* clears, int n_clears,
             int32_t* d_owner, mcpt_stats* stats, hipStream_t st, const MapAnswer& answer)
{
    if (const int rc = lightmap_device_gate(d)) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    const size_t n = size_t(W) * H, ch = size_t(channels);
    LightmapWork w{};
    Lease l;                                                // (d->lm's: the query behind `answer` holds its own)
    if (const int rc = lightmap_ensure_work(d, W, H, w, st, l)) return rc;
    mcpt_device::Lightmap& m = *d->lm;
    if (R > 0) {
        if (const int rc = grow(m.owner[1], n, kWork)) return rc;
        if (const int rc = grow(m.irr, n * ch, kWork)) return rc;
    }
    int32_t covered = 0;
    if (const int rc = lightmap_raster_device(d, d_uv6, W, H, w, st, covered)) return rc;
    // the rounds alternate between the caller's frame and the baker's own: the scatter starts where R rounds end in the caller's
    double* const frame[2] = {d_map, m.irr.get()};
    int at = R & 1;
    HIP_TRY(hipMemsetAsync(frame[at], 0, n * ch * sizeof(double), st));
    for (int i = 0; i < n_clears; i++)
        if (clears[i].map) HIP_TRY(hipMemsetAsync(clears[i].map, 0, clears[i].bytes, st));
    if (covered > 0) {
        const size_t c = size_t(covered);
        if (const int rc = grow(m.texels, c, kWork)) return rc;
        if (const int rc = grow(m.q6, c * 6, kWork)) return rc;
        launch_lightmap_texels(d->ds, d_uv6, W, H, w, m.texels.get(), m.q6.get(), st);
        HIP_TRY(hipGetLastError());
        if (const int rc = answer(m.texels.get(), m.q6.get(), covered, frame[at])) return rc;
        HIP_TRY(hipGetLastError());
    }
    int32_t* const own[2] = {m.owner[0].get(), m.owner[1].get()};
    lightmap_dilate_rounds(frame, own, W, H, R, channels, at, st);
    HIP_TRY(hipGetLastError());
    if (d_owner) HIP_TRY(hipMemcpyAsync(d_owner, own[R & 1], n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return l.end(MCPT_OK);
}

// Both irradiance bakes on st, after the refusals; device pointers throughout.  ap: an adaptive bake (mcpt_bake_lightmap_adaptive) -- step 3
// is the adaptive query call (adaptive_query_api.cpp) and d_counts (may be null) the map of the texels' own sample counts; null: a
// uniform bake, step 3 the query call (query_api.cpp).
static int bake_device(mcpt_device* d, const double* d_uv6, const mcpt_lightmap_params& p, const mcpt_adaptive_params* ap, double* d_irr, double* d_err,
                       int32_t* d_hits, int32_t* d_owner, int32_t* d_counts, mcpt_stats* stats, hipStream_t st)
{
    const size_t n = size_t(p.width) * p.height;
    const MapClear clears[] = {{d_err, n * 3 * sizeof(double)}, {d_hits, n * sizeof(int32_t)}, {d_counts, n * sizeof(int32_t)}};
    return map_bake(d, d_uv6, p.width, p.height, p.dilate, 3, d_irr, clears, 3, d_owner, stats, st,
                    [&](const int32_t* texels, const double* q6, int32_t covered, double* frame_at) -> int {
        const size_t c = size_t(covered);
        mcpt_device::Lightmap& m = *d->lm;
        if (const int rc = grow(m.mean, c * 3, kWork)) return rc;
        if (d_err)
            if (const int rc = grow(m.err, c * 3, kWork)) return rc;
        if (d_hits)
            if (const int rc = grow(m.hits, c, kWork)) return rc;
        if (d_counts)
            if (const int rc = grow(m.counts, c, kWork)) return rc;
        const DQuery q{q6, MCPT_QUERY_HEMISPHERE, m.mean.get(), d_err ? m.err.get() : nullptr, d_hits ? m.hits.get() : nullptr};
        if (ap) {
            if (const int rc = adaptive_query_device(d, q, texels, covered, p.spp, p.sample_base, p.seed, p.flags, *ap, d_counts ? m.counts.get() : nullptr,
                                                     stats, st))
                return rc;
            if (d_counts) launch_aq_scatter_counts(texels, covered, m.counts.get(), d_counts, st);
        } else if (const int rc = query_device(d, q, texels, covered, p.spp, p.sample_base, p.seed, p.flags, stats, st)) return rc;
        launch_lightmap_scatter(texels, covered, q.mean3, q.stderr3, q.hits, frame_at, d_err, d_hits, st);
        return MCPT_OK;
    });
}

extern "C" {

int mcpt_lightmap_raster_host(const double* uv6, int64_t num_faces, int32_t width, int32_t height, int32_t* owner)
{
    if (num_faces < 0 || num_faces > 0x7ffffffe) return fail(MCPT_ERR_ARG, "the number of faces must be in 0 .. 2^31 - 2");
    if (const int rc = lightmap_size_check(width, height)) return rc;
    if (!owner || (num_faces > 0 && !uv6)) return fail(MCPT_ERR_ARG, "null argument");
    if (const int rc = lightmap_chart_check(uv6, num_faces)) return rc;
    const size_t n = size_t(width) * height;
    for (size_t i = 0; i < n; i++) owner[i] = -1;
    // faces in descending order, so that the lowest face that covers a texel is the last to write it
    for (int64_t f = num_faces - 1; f >= 0; f--) {
        const double* uv = uv6 + f * 6;
        const double area2 = lightmap_area2(uv);
        if (!lightmap_area_ok(area2)) continue;
        int x0, x1, y0, y1;
        if (!lightmap_box(uv, width, height, x0, x1, y0, y1)) continue;
        for (int y = y0; y <= y1; y++) {
            const double pv = lightmap_centre(y, height);
            for (int x = x0; x <= x1; x++) {
                double e[3];
                lightmap_edges(uv, lightmap_centre(x, width), pv, e);
                if (lightmap_covers(area2, e)) owner[size_t(y) * width + x] = int32_t(f);
            }
        }
    }
    return MCPT_OK;
}

int64_t mcpt_lightmap_texels(mcpt_device* d, const double* uv6, int32_t width, int32_t height, int32_t* owner, int32_t* texels, double* q6, int64_t cap)
{
    if (const int rc = lightmap_size_check(width, height)) return rc;
    if (cap < 0) return fail(MCPT_ERR_ARG, "cap must be >= 0");
    if (const int rc = device_gate(d)) return rc;
    if (uv6)
        if (const int rc = lightmap_chart_check(uv6, d->ds.t)) return rc;
    if (const int rc = motion_home(d)) return rc;
    if (const int rc = geometry_gate(d)) return rc;
    hipStream_t st = d->stream.get();
    Staging S(st);
    const double* d_uv = nullptr;                           // (null stays null: the scene's own vt)
    if (const int rc = S.in(uv6, size_t(d->ds.t) * 6, "the chart", d_uv)) return rc;
    LightmapWork w{};
    Lease l;
    if (const int rc = lightmap_ensure_work(d, width, height, w, st, l)) return rc;
    int32_t covered = 0;
    if (const int rc = lightmap_raster_device(d, d_uv, width, height, w, st, covered)) return rc;
    const size_t n = size_t(width) * height, c = size_t(covered);
    if ((texels || q6) && covered > cap) return fail(MCPT_ERR_ARG, "more texels are covered (" + std::to_string(covered) + ") than the list holds");
    if (owner) HIP_TRY(hipMemcpy(owner, w.owner, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if ((texels || q6) && covered > 0) {
        int32_t* d_texels = nullptr;
        double* d_q6 = nullptr;
        if (const int rc = S.out(texels, c, "the texel list", d_texels)) return rc;
        if (const int rc = S.out(q6, c * 6, "the texels' surface points", d_q6)) return rc;
        launch_lightmap_texels(d->ds, d_uv, width, height, w, d_texels, d_q6, st);
        if (const int rc = S.finish(launch_result())) return rc;
    }
    return covered;
}

int mcpt_bake_lightmap_device(mcpt_device* d, const double* d_uv6, const mcpt_lightmap_params* p, double* d_irradiance3, double* d_stderr3,
                              int32_t* d_hits, int32_t* d_owner, mcpt_stats* stats, void* stream)
{
    if (const int rc = params_check(p, d_irradiance3)) return rc;
    return bake_device(d, d_uv6, *p, nullptr, d_irradiance3, d_stderr3, d_hits, d_owner, nullptr, stats, static_cast<hipStream_t>(stream));
}

}  // extern "C"

// the host-pointer form of both bakes, after their refusals (ap null: the uniform one)
static int bake_host(mcpt_device* d, const double* uv6, const mcpt_lightmap_params* p, const mcpt_adaptive_params* ap, double* irradiance3, double* stderr3,
                     int32_t* hits, int32_t* owner, int32_t* counts, mcpt_stats* stats)
{
    if (const int rc = device_gate(d)) return rc;
    if (uv6)
        if (const int rc = lightmap_chart_check(uv6, d->ds.t)) return rc;
    const size_t n = size_t(p->width) * p->height;
    Staging S(d->stream.get());
    const double* d_uv = nullptr;                           // (null stays null: the scene's own vt)
    double *d_irr = nullptr, *d_err = nullptr;
    int32_t *d_hits = nullptr, *d_owner = nullptr, *d_counts = nullptr;
    if (const int rc = S.in(uv6, size_t(d->ds.t) * 6, "the chart", d_uv)) return rc;
    if (const int rc = S.out(irradiance3, n * 3, "the irradiance map", d_irr)) return rc;
    if (const int rc = S.out(stderr3, n * 3, "the standard error map", d_err)) return rc;
    if (const int rc = S.out(hits, n, "the hit map", d_hits)) return rc;
    if (const int rc = S.out(owner, n, "the owner map", d_owner)) return rc;
    if (const int rc = S.out(counts, n, "the sample count map", d_counts)) return rc;
    return S.finish(bake_device(d, d_uv, *p, ap, d_irr, d_err, d_hits, d_owner, d_counts, stats, d->stream.get()));
}

extern "C" {

int mcpt_bake_lightmap(mcpt_device* d, const double* uv6, const mcpt_lightmap_params* p, double* irradiance3, double* stderr3, int32_t* hits,
                       int32_t* owner, mcpt_stats* stats)
{
    if (const int rc = params_check(p, irradiance3)) return rc;
    return bake_host(d, uv6, p, nullptr, irradiance3, stderr3, hits, owner, nullptr, stats);
}

int mcpt_bake_lightmap_adaptive_device(mcpt_device* d, const double* d_uv6, const mcpt_lightmap_params* p, const mcpt_adaptive_params* ap,
                                       double* d_irradiance3, double* d_stderr3, int32_t* d_hits, int32_t* d_owner, int32_t* d_counts, mcpt_stats* stats,
                                       void* stream)
{
    if (const int rc = params_check(p, d_irradiance3)) return rc;
    if (const int rc = adaptive_params_check(ap)) return rc;
    return bake_device(d, d_uv6, *p, ap, d_irradiance3, d_stderr3, d_hits, d_owner, d_counts, stats, static_cast<hipStream_t>(stream));
}

int mcpt_bake_lightmap_adaptive(mcpt_device* d, const double* uv6, const mcpt_lightmap_params* p, const mcpt_adaptive_params* ap, double* irradiance3,
                                double* stderr3, int32_t* hits, int32_t* owner, int32_t* counts, mcpt_stats* stats)
{
    if (const int rc = params_check(p, irradiance3)) return rc;
    if (const int rc = adaptive_params_check(ap)) return rc;
    return bake_host(d, uv6, p, ap, irradiance3, stderr3, hits, owner, counts, stats);
}

}  // extern "C"
