// C ABI, baked frames (include/mcpt.h: mcpt_lightmap_irradiance*, mcpt_baked_radiance*, mcpt_render_baked*): the lightmap's lookup by chart
// coordinate, and camera or caller's rays shaded from a bake.  A call writes or takes the rays of a chunk, answers them with the unchanged
// closest-hit launch (kernels.hip: launch_trace_closest_leaf -- mcpt_trace_closest_device's walks, handing back the leaf), shades the hits
// under the source (baked.hip) and, a frame, folds every pixel's samples.  The workspace is the device's own (mcpt_device::Baked).  The
// lookup's arithmetic is baked.hpp's, compiled here for the host form.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>
#include <limits>
#include <string>

#include "baked.hpp"
#include "handles.hpp"

using namespace mcpt;

static constexpr int64_t kInt32Max = std::numeric_limits<int32_t>::max();
static constexpr int64_t kDefaultWorkspaceRays = int64_t(1) << 22;  // 487 MB of workspace
static constexpr int32_t kMaxSamples = 65536;
static constexpr size_t kRayBytes = (6 + 1 + 3 + 3) * sizeof(double) + 3 * sizeof(int32_t);
static_assert(kRayBytes == 116, "mcpt.h states the workspace's bytes per ray");

// what every form of the lightmap lookup refuses without looking at the arrays
static int lookup_check(int32_t W, int32_t H, const void* irr, const void* uv2, int64_t n, const void* e3)
{
    if (const int rc = lightmap_size_check(W, H)) return rc;
    if (n < 0 || n > kInt32Max) return fail(MCPT_ERR_ARG, "the number of chart coordinates must be in 0 .. 2^31 - 1");
    if (n > 0 && (!irr || !uv2 || !e3)) return fail(MCPT_ERR_ARG, "null irradiance map, chart coordinates or irradiance");
    return MCPT_OK;
}

// ... and what the host-pointer forms refuse of the coordinates themselves
static int lookup_uv_check(const double* uv2, int64_t n)
{
    for (int64_t i = 0; i < n * 2; i++)
        if (!std::isfinite(uv2[i])) return fail(MCPT_ERR_ARG, "chart coordinate " + std::to_string(i / 2) + ": component that is not finite");
    return MCPT_OK;
}

// what every call refuses of its source, in the header's order
static int source_check(const mcpt_baked_source* s)
{
    if (!s) return fail(MCPT_ERR_ARG, "null baked source");
    if (s->kind != MCPT_BAKED_VOLUME && s->kind != MCPT_BAKED_LIGHTMAP) return fail(MCPT_ERR_ARG, "a baked source is MCPT_BAKED_VOLUME or MCPT_BAKED_LIGHTMAP");
    if (s->flags != 0) return fail(MCPT_ERR_ARG, "mcpt_baked_source.flags must be 0");
    for (int i = 0; i < 4; i++)
        if (s->reserved[i] != 0) return fail(MCPT_ERR_ARG, "mcpt_baked_source.reserved must be 0");
    if (s->kind == MCPT_BAKED_VOLUME) {
        if (const int rc = volume_grid_check(s->grid)) return rc;
        if (!s->sh27) return fail(MCPT_ERR_ARG, "null coefficients");
        if (s->moments)
            if (const int rc = volume_visibility_check(s->visibility)) return rc;
    } else {
        if (const int rc = lightmap_size_check(s->width, s->height)) return rc;
        if (!s->irradiance3) return fail(MCPT_ERR_ARG, "null irradiance map");
    }
    return MCPT_OK;
}

static int radiance_check(const mcpt_baked_source* s, const void* rays6, int64_t n, int32_t flags, const mcpt_baked_outputs* o)
{
    if (const int rc = source_check(s)) return rc;
    if (flags & ~(MCPT_BAKED_FACE_VIEWER | MCPT_BAKED_LIGHTING_ONLY)) return fail(MCPT_ERR_ARG, "unknown baked flag");
    if (n < 0 || n > kInt32Max) return fail(MCPT_ERR_ARG, "the number of rays must be in 0 .. 2^31 - 1");
    if (n > 0 && !rays6) return fail(MCPT_ERR_ARG, "null rays");
    if (!o) return fail(MCPT_ERR_ARG, "null baked outputs");
    if (o->reserved[0] != 0 || o->reserved[1] != 0) return fail(MCPT_ERR_ARG, "mcpt_baked_outputs.reserved must be 0");
    return MCPT_OK;
}

static int frame_check(const mcpt_baked_source* s, const mcpt_baked_frame_params* p, const void* img)
{
    if (const int rc = source_check(s)) return rc;
    if (!p) return fail(MCPT_ERR_ARG, "null baked frame parameters");
    if (p->samples < 1 || p->samples > kMaxSamples) return fail(MCPT_ERR_ARG, "samples must be in 1 .. 65536");
    if (p->flags & ~(MCPT_BAKED_FACE_VIEWER | MCPT_BAKED_LIGHTING_ONLY)) return fail(MCPT_ERR_ARG, "unknown baked flag");
    if (p->workspace_rays < 0) return fail(MCPT_ERR_ARG, "workspace_rays must be >= 0");
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(MCPT_ERR_ARG, "mcpt_baked_frame_params.reserved must be 0");
    if (!img) return fail(MCPT_ERR_ARG, "null image");
    return MCPT_OK;
}

// a checked source whose pointers are the device's, as the kernels read it
static BakedSource device_source(const mcpt_baked_source& s)
{
    BakedSource B{};
    B.kind = s.kind;
    if (s.kind == MCPT_BAKED_VOLUME) {
        B.grid = *s.grid;
        B.sh27 = s.sh27; B.valid = s.valid;
        if (s.moments) { B.visible = 1; B.vis = *s.visibility; B.moments = s.moments; }
    } else {
        B.uv6 = s.uv6; B.width = s.width; B.height = s.height; B.irr = s.irradiance3; B.owner = s.owner;
    }
    return B;
}

// The device copies of a host-pointer source.
struct SourceCopy {
    DevBuf<double> sh, moments, uv, irr;
    DevBuf<uint8_t> valid;
    DevBuf<int32_t> owner;
    mcpt_baked_source dev{};
};
template <class T>
static int upload(DevBuf<T>& b, const T* host, size_t count, const char* what)
{
    const size_t bytes = (count > 0 ? count : 1) * sizeof(T);
    if (const int rc = volume_alloc_result(b.alloc_bytes(bytes), what, bytes)) return rc;
    if (count > 0) HIP_TRY(hipMemcpy(b.get(), host, count * sizeof(T), hipMemcpyHostToDevice));
    return MCPT_OK;
}
static int source_upload(const mcpt_device* d, const mcpt_baked_source& s, SourceCopy& c)
{
    c.dev = s;
    if (s.kind == MCPT_BAKED_VOLUME) {
        const size_t probes = size_t(volume_probes(*s.grid));
        if (const int rc = upload(c.sh, s.sh27, probes * MCPT_SH_N * 3, "the volume's coefficients")) return rc;
        c.dev.sh27 = c.sh.get();
        if (s.valid) {
            if (const int rc = upload(c.valid, s.valid, probes, "the volume's mask")) return rc;
            c.dev.valid = c.valid.get();
        }
        if (s.moments) {
            const size_t bins = size_t(s.visibility->res) * size_t(s.visibility->res);
            if (const int rc = upload(c.moments, s.moments, probes * bins * 2, "the volume's moments")) return rc;
            c.dev.moments = c.moments.get();
        }
    } else {
        const size_t texels = size_t(s.width) * size_t(s.height);
        if (s.uv6) {
            if (const int rc = lightmap_chart_check(s.uv6, d->ds.t)) return rc;
            if (const int rc = upload(c.uv, s.uv6, size_t(d->ds.t) * 6, "the chart")) return rc;
            c.dev.uv6 = c.uv.get();
        }
        if (const int rc = upload(c.irr, s.irradiance3, texels * 3, "the irradiance map")) return rc;
        c.dev.irradiance3 = c.irr.get();
        if (s.owner) {
            if (const int rc = upload(c.owner, s.owner, texels, "the owner map")) return rc;
            c.dev.owner = c.owner.get();
        }
    }
    return MCPT_OK;
}

// what every baked call on a device asks before it reads the device's triangles, and the workspace for chunks of `rays` rays once the call
// before this one has left it
static int baked_gate(mcpt_device* d)
{
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    HIP_TRY(hipSetDevice(d->ordinal));
    return MCPT_OK;
}
static int baked_workspace(mcpt_device* d, int64_t rays, bool own_rays, bool samples)
{
    if (!d->baked) {
        auto b = std::make_unique<mcpt_device::Baked>();
        HIP_TRY(create(b->done, hipEventCreateWithFlags, hipEventDisableTiming));
        d->baked = std::move(b);
    }
    mcpt_device::Baked& w = *d->baked;
    HIP_TRY(hipEventSynchronize(w.done.get()));             // the call before this one has left the workspace
    if (rays > (int64_t(1) << 40)) return fail(MCPT_ERR_NOMEM, "the baked workspace of " + std::to_string(rays) + " rays cannot be allocated");
    const size_t sr = size_t(rays);
    if (own_rays)
        if (const int rc = volume_alloc_result(w.rays6.grow_bytes(sr * 6 * sizeof(double)), "the baked rays", sr * 6 * sizeof(double))) return rc;
    if (const int rc = volume_alloc_result(w.t.grow_bytes(sr * sizeof(double)), "the baked rays' distances", sr * sizeof(double))) return rc;
    if (const int rc = volume_alloc_result(w.p.grow_bytes(sr * 3 * sizeof(double)), "the baked rays' hit points", sr * 3 * sizeof(double))) return rc;
    if (const int rc = volume_alloc_result(w.leaf.grow_bytes(sr * sizeof(int32_t)), "the baked rays' hits", sr * sizeof(int32_t))) return rc;
    if (samples) {
        if (const int rc = volume_alloc_result(w.rad.grow_bytes(sr * 3 * sizeof(double)), "the baked samples' radiance", sr * 3 * sizeof(double))) return rc;
        if (const int rc = volume_alloc_result(w.kind.grow_bytes(sr * sizeof(int32_t)), "the baked samples' kinds", sr * sizeof(int32_t))) return rc;
        if (const int rc = volume_alloc_result(w.lit.grow_bytes(sr * sizeof(int32_t)), "the baked samples' lookups", sr * sizeof(int32_t))) return rc;
    }
    return MCPT_OK;
}

static inline void trace_chunk(mcpt_device* d, const double* d_rays6, int64_t n, hipStream_t st)
{
    mcpt_device::Baked& w = *d->baked;
    launch_trace_closest_leaf(d->ds, d->trace_mode == MCPT_TRACE_FAST, d_rays6, n, w.leaf.get(), w.t.get(), w.p.get(), d->aux_ctr.get(), d->aux_queue.get(),
                              d->aux_slow_list.get(), d->slow_cap, st, d->cfg);
}

// the outputs of rays first .. of a call
static BakedOut outputs_at(const mcpt_baked_outputs& o, int64_t first)
{
    BakedOut r{};
    r.radiance3 = o.radiance3 ? o.radiance3 + first * 3 : nullptr;
    r.kind = o.kind ? o.kind + first : nullptr;
    r.face = o.face ? o.face + first : nullptr;
    r.q6 = o.q6 ? o.q6 + first * 6 : nullptr;
    r.uv2 = o.uv2 ? o.uv2 + first * 2 : nullptr;
    r.kd3 = o.kd3 ? o.kd3 + first * 3 : nullptr;
    r.e3 = o.e3 ? o.e3 + first * 3 : nullptr;
    r.lit = o.lit ? o.lit + first : nullptr;
    return r;
}

// Baked radiance on st, after the refusals and the gate; device pointers throughout.  Nothing here waits for st unless the caller asks for
// statistics.
static int radiance_device(mcpt_device* d, const mcpt_baked_source& s, const double* d_rays6, int64_t n, int32_t flags, const mcpt_baked_outputs& o,
                           mcpt_stats* stats, hipStream_t st)
{
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return MCPT_OK;
    if (const int rc = motion_home(d)) return rc;           // a device that holds a motion answers from key 0
    if (const int rc = geometry_gate(d)) return rc;
    const int64_t per_chunk = n < kDefaultWorkspaceRays ? n : kDefaultWorkspaceRays;
    if (const int rc = baked_workspace(d, per_chunk, false, false)) return rc;
    mcpt_device::Baked& w = *d->baked;
    const BakedSource B = device_source(s);
    int chunks = 0;
    int rc = MCPT_OK;
    for (int64_t first = 0; first < n && rc == MCPT_OK; first += per_chunk, chunks++) {
        const int64_t count = n - first < per_chunk ? n - first : per_chunk;
        const double* rays = d_rays6 + first * 6;
        trace_chunk(d, rays, count, st);
        launch_baked_shade(d->ds, B, flags, rays, w.leaf.get(), w.t.get(), w.p.get(), count, outputs_at(o, first), st);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = fail(MCPT_ERR_HIP, hipGetErrorString(e));
    }
    HIP_TRY(hipEventRecord(w.done.get(), st));              // also after a failure: kernels may be enqueued
    if (rc != MCPT_OK) return rc;
    if (stats) {
        HIP_TRY(hipStreamSynchronize(st));
        stats->rays_primary = stats->samples = uint64_t(n);
        stats->launches = chunks;
    }
    return MCPT_OK;
}

// A baked frame on st, after the refusals and the gate; device pointers throughout.
static int frame_device(mcpt_device* d, const mcpt_baked_source& s, const mcpt_baked_frame_params& fp, double* d_img, int32_t* d_counts3, int32_t* d_lit,
                        mcpt_stats* stats, hipStream_t st)
{
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (const int rc = motion_home(d)) return rc;
    if (const int rc = geometry_gate(d)) return rc;
    const int64_t pixels = int64_t(d->width) * d->height;
    if (pixels == 0) return MCPT_OK;
    if (const int rc = ensure_pos(d, st)) return rc;
    const int G = fp.samples;
    const int flags = fp.flags;
    const int64_t budget = fp.workspace_rays > 0 ? fp.workspace_rays : kDefaultWorkspaceRays;
    int64_t per_chunk = budget / G;                         // whole pixels, at least one
    per_chunk = per_chunk < 1 ? 1 : (per_chunk > pixels ? pixels : per_chunk);
    if (const int rc = baked_workspace(d, per_chunk * G, true, true)) return rc;
    mcpt_device::Baked& w = *d->baked;
    const BakedSource B = device_source(s);
    const DLens lens = lens_for(d, d->lens);
    int chunks = 0;
    int rc = MCPT_OK;
    for (int64_t first = 0; first < pixels && rc == MCPT_OK; first += per_chunk, chunks++) {
        BakedChunk c{};
        c.first = int(first); c.n = int(pixels - first < per_chunk ? pixels - first : per_chunk); c.G = G;
        c.rays6 = w.rays6.get(); c.leaf = w.leaf.get(); c.t = w.t.get(); c.p = w.p.get();
        const long long rays = (long long)c.n * G;
        launch_baked_camera_rays(lens, fp.seed, c, w.rays6.get(), st);
        trace_chunk(d, c.rays6, rays, st);
        BakedOut o{};
        o.radiance3 = w.rad.get(); o.kind = w.kind.get(); o.lit = w.lit.get();
        launch_baked_shade(d->ds, B, flags, c.rays6, c.leaf, c.t, c.p, rays, o, st);
        launch_baked_fold(c, w.rad.get(), w.kind.get(), w.lit.get(), d_img, d_counts3, d_lit, st);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = fail(MCPT_ERR_HIP, hipGetErrorString(e));
    }
    HIP_TRY(hipEventRecord(w.done.get(), st));              // also after a failure: kernels may be enqueued
    if (rc != MCPT_OK) return rc;
    if (stats) {
        HIP_TRY(hipStreamSynchronize(st));
        stats->rays_primary = stats->samples = uint64_t(pixels) * uint64_t(G);
        stats->launches = chunks;
    }
    return MCPT_OK;
}

// the end of a host-pointer call: the stream is waited for, on failure as well -- nothing enqueued may still use a copy when it goes
static int finish(int rc, hipStream_t st)
{
    const hipError_t e = hipStreamSynchronize(st);
    if (rc == MCPT_OK && e != hipSuccess) rc = fail(MCPT_ERR_HIP, hipGetErrorString(e));
    return rc;
}

extern "C" {

int mcpt_lightmap_irradiance_host(int32_t width, int32_t height, const double* irradiance3, const int32_t* owner, const double* uv2, int64_t n, double* e3,
                                  int32_t* taps)
{
    if (const int rc = lookup_check(width, height, irradiance3, uv2, n, e3)) return rc;
    if (const int rc = lookup_uv_check(uv2, n)) return rc;
    for (int64_t i = 0; i < n; i++) {
        const int c = baked_lightmap_lookup(width, height, irradiance3, owner, uv2[i * 2], uv2[i * 2 + 1], e3 + i * 3);
        if (taps) taps[i] = c;
    }
    return MCPT_OK;
}

int mcpt_lightmap_irradiance_device(mcpt_device* d, int32_t width, int32_t height, const double* d_irradiance3, const int32_t* d_owner, const double* d_uv2,
                                    int64_t n, double* d_e3, int32_t* d_taps, void* stream)
{
    if (const int rc = lookup_check(width, height, d_irradiance3, d_uv2, n, d_e3)) return rc;
    if (const int rc = baked_gate(d)) return rc;
    if (n == 0) return MCPT_OK;
    launch_lightmap_irradiance(width, height, d_irradiance3, d_owner, d_uv2, n, d_e3, d_taps, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return MCPT_OK;
}

int mcpt_lightmap_irradiance(mcpt_device* d, int32_t width, int32_t height, const double* irradiance3, const int32_t* owner, const double* uv2, int64_t n,
                             double* e3, int32_t* taps)
{
    if (const int rc = lookup_check(width, height, irradiance3, uv2, n, e3)) return rc;
    if (const int rc = lookup_uv_check(uv2, n)) return rc;
    if (const int rc = baked_gate(d)) return rc;
    if (n == 0) return MCPT_OK;
    const size_t texels = size_t(width) * size_t(height), sn = size_t(n);
    DevBuf<double> d_irr, d_uv, d_e;
    DevBuf<int32_t> d_owner, d_taps;
    if (const int rc = upload(d_irr, irradiance3, texels * 3, "the irradiance map")) return rc;
    if (owner)
        if (const int rc = upload(d_owner, owner, texels, "the owner map")) return rc;
    if (const int rc = upload(d_uv, uv2, sn * 2, "the chart coordinates")) return rc;
    if (const int rc = volume_alloc_result(d_e.alloc_bytes(sn * 3 * sizeof(double)), "the coordinates' irradiance", sn * 3 * sizeof(double))) return rc;
    if (taps) HIP_TRY(d_taps.alloc(sn));
    hipStream_t st = d->stream.get();
    launch_lightmap_irradiance(width, height, d_irr.get(), owner ? d_owner.get() : nullptr, d_uv.get(), n, d_e.get(), taps ? d_taps.get() : nullptr, st);
    const hipError_t el = hipGetLastError();
    if (const int rc = finish(el == hipSuccess ? MCPT_OK : fail(MCPT_ERR_HIP, hipGetErrorString(el)), st)) return rc;
    HIP_TRY(hipMemcpy(e3, d_e.get(), sn * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (taps) HIP_TRY(hipMemcpy(taps, d_taps.get(), sn * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MCPT_OK;
}

int mcpt_baked_radiance_device(mcpt_device* d, const mcpt_baked_source* s, const double* d_rays6, int64_t n, int32_t flags, const mcpt_baked_outputs* o,
                               mcpt_stats* stats, void* stream)
{
    if (const int rc = radiance_check(s, d_rays6, n, flags, o)) return rc;
    if (const int rc = baked_gate(d)) return rc;
    return radiance_device(d, *s, d_rays6, n, flags, *o, stats, static_cast<hipStream_t>(stream));
}

int mcpt_baked_radiance(mcpt_device* d, const mcpt_baked_source* s, const double* rays6, int64_t n, int32_t flags, const mcpt_baked_outputs* o,
                        mcpt_stats* stats)
{
    if (const int rc = radiance_check(s, rays6, n, flags, o)) return rc;
    if (const int rc = baked_gate(d)) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    SourceCopy sc;
    if (const int rc = source_upload(d, *s, sc)) return rc;
    if (n == 0) return MCPT_OK;
    const size_t sn = size_t(n);
    DevBuf<double> d_rays, d_rad, d_q, d_uv, d_kd, d_e;
    DevBuf<int32_t> d_kind, d_face, d_lit;
    if (const int rc = upload(d_rays, rays6, sn * 6, "the rays")) return rc;
    mcpt_baked_outputs dev{};
    // one device array per output the caller asks for
    auto want_d = [&](double* host, DevBuf<double>& b, size_t per, double*& slot) -> int {
        if (!host) return MCPT_OK;
        if (const int rc = volume_alloc_result(b.alloc_bytes(sn * per * sizeof(double)), "a baked output", sn * per * sizeof(double))) return rc;
        slot = b.get();
        return MCPT_OK;
    };
    auto want_i = [&](int32_t* host, DevBuf<int32_t>& b, int32_t*& slot) -> int {
        if (!host) return MCPT_OK;
        if (const int rc = volume_alloc_result(b.alloc_bytes(sn * sizeof(int32_t)), "a baked output", sn * sizeof(int32_t))) return rc;
        slot = b.get();
        return MCPT_OK;
    };
    if (const int rc = want_d(o->radiance3, d_rad, 3, dev.radiance3)) return rc;
    if (const int rc = want_i(o->kind, d_kind, dev.kind)) return rc;
    if (const int rc = want_i(o->face, d_face, dev.face)) return rc;
    if (const int rc = want_d(o->q6, d_q, 6, dev.q6)) return rc;
    if (const int rc = want_d(o->uv2, d_uv, 2, dev.uv2)) return rc;
    if (const int rc = want_d(o->kd3, d_kd, 3, dev.kd3)) return rc;
    if (const int rc = want_d(o->e3, d_e, 3, dev.e3)) return rc;
    if (const int rc = want_i(o->lit, d_lit, dev.lit)) return rc;
    hipStream_t st = d->stream.get();
    if (const int rc = finish(radiance_device(d, sc.dev, d_rays.get(), n, flags, dev, stats, st), st)) return rc;
    if (o->radiance3) HIP_TRY(hipMemcpy(o->radiance3, dev.radiance3, sn * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (o->kind) HIP_TRY(hipMemcpy(o->kind, dev.kind, sn * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (o->face) HIP_TRY(hipMemcpy(o->face, dev.face, sn * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (o->q6) HIP_TRY(hipMemcpy(o->q6, dev.q6, sn * 6 * sizeof(double), hipMemcpyDeviceToHost));
    if (o->uv2) HIP_TRY(hipMemcpy(o->uv2, dev.uv2, sn * 2 * sizeof(double), hipMemcpyDeviceToHost));
    if (o->kd3) HIP_TRY(hipMemcpy(o->kd3, dev.kd3, sn * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (o->e3) HIP_TRY(hipMemcpy(o->e3, dev.e3, sn * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (o->lit) HIP_TRY(hipMemcpy(o->lit, dev.lit, sn * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MCPT_OK;
}

int mcpt_render_baked_device(mcpt_device* d, const mcpt_baked_source* s, const mcpt_baked_frame_params* p, double* d_img, int32_t* d_counts3, int32_t* d_lit,
                             mcpt_stats* stats, void* stream)
{
    if (const int rc = frame_check(s, p, d_img)) return rc;
    if (const int rc = baked_gate(d)) return rc;
    return frame_device(d, *s, *p, d_img, d_counts3, d_lit, stats, static_cast<hipStream_t>(stream));
}

int mcpt_render_baked(mcpt_device* d, const mcpt_baked_source* s, const mcpt_baked_frame_params* p, double* img, int32_t* counts3, int32_t* lit,
                      mcpt_stats* stats)
{
    if (const int rc = frame_check(s, p, img)) return rc;
    if (const int rc = baked_gate(d)) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    SourceCopy sc;
    if (const int rc = source_upload(d, *s, sc)) return rc;
    const size_t px = size_t(d->width) * size_t(d->height);
    if (px == 0) return MCPT_OK;
    DevBuf<double> d_img;
    DevBuf<int32_t> d_counts, d_lit;
    if (const int rc = volume_alloc_result(d_img.alloc_bytes(px * 3 * sizeof(double)), "the frame", px * 3 * sizeof(double))) return rc;
    if (counts3) HIP_TRY(d_counts.alloc(px * 3));
    if (lit) HIP_TRY(d_lit.alloc(px));
    hipStream_t st = d->stream.get();
    if (const int rc = finish(frame_device(d, sc.dev, *p, d_img.get(), counts3 ? d_counts.get() : nullptr, lit ? d_lit.get() : nullptr, stats, st), st)) return rc;
    HIP_TRY(hipMemcpy(img, d_img.get(), px * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (counts3) HIP_TRY(hipMemcpy(counts3, d_counts.get(), px * 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (lit) HIP_TRY(hipMemcpy(lit, d_lit.get(), px * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MCPT_OK;
}

}  // extern "C"
