// C ABI, baked frames (include/mcpt.h: mcpt_lightmap_irradiance*, mcpt_baked_radiance*, mcpt_render_baked*): the lightmap's lookup by chart
// coordinate, and camera or caller's rays shaded from a bake.  A call writes or takes the rays of a chunk, answers them with the unchanged
// closest-hit launch (hit_work.hpp: trace_leaf -- mcpt_trace_closest_device's walks, handing back the leaf), shades the hits
// under the source (baked.hip) and, a frame, folds every pixel's samples.  The workspace is the device's own (mcpt_device::Baked).  The
// lookup's arithmetic is baked.hpp's, compiled here for the host form.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>
#include <string>

#include "baked.hpp"
#include "baked_specular.hpp"
#include "chunks.hpp"
#include "handles.hpp"

using namespace mcpt;

static constexpr int32_t kMaxSamples = 65536;
static constexpr size_t kRayBytes = (6 + 1 + 3 + 3) * sizeof(double) + 3 * sizeof(int32_t);
static_assert(kRayBytes == 116, "mcpt.h states the workspace's bytes per ray");   // (the default workspace of 2^22 rays: 487 MB)

// what every form of the lightmap lookup refuses without looking at the arrays
static int lookup_check(int32_t W, int32_t H, const void* irr, const void* uv2, int64_t n, const void* e3)
{
    if (const int rc = lightmap_size_check(W, H)) return rc;
    if (const int rc = count_check(n, "chart coordinates")) return rc;
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
int baked_source_check(const mcpt_baked_source* s)
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

// what a baked radiance call refuses of its own arguments, after its source
int baked_radiance_args_check(const void* rays6, int64_t n, int32_t flags, const mcpt_baked_outputs* o)
{
    if (flags & ~(MCPT_BAKED_FACE_VIEWER | MCPT_BAKED_LIGHTING_ONLY)) return fail(MCPT_ERR_ARG, "unknown baked flag");
    if (const int rc = count_check(n, "rays")) return rc;
    if (n > 0 && !rays6) return fail(MCPT_ERR_ARG, "null rays");
    if (!o) return fail(MCPT_ERR_ARG, "null baked outputs");
    if (o->reserved[0] != 0 || o->reserved[1] != 0) return fail(MCPT_ERR_ARG, "mcpt_baked_outputs.reserved must be 0");
    return MCPT_OK;
}

static int radiance_check(const mcpt_baked_source* s, const void* rays6, int64_t n, int32_t flags, const mcpt_baked_outputs* o)
{
    if (const int rc = baked_source_check(s)) return rc;
    return baked_radiance_args_check(rays6, n, flags, o);
}

// what a baked frame call refuses of its own arguments, after its source
int baked_frame_args_check(const mcpt_baked_frame_params* p, const void* img)
{
    if (!p) return fail(MCPT_ERR_ARG, "null baked frame parameters");
    if (p->samples < 1 || p->samples > kMaxSamples) return fail(MCPT_ERR_ARG, "samples must be in 1 .. 65536");
    if (p->flags & ~(MCPT_BAKED_FACE_VIEWER | MCPT_BAKED_LIGHTING_ONLY)) return fail(MCPT_ERR_ARG, "unknown baked flag");
    if (p->workspace_rays < 0) return fail(MCPT_ERR_ARG, "workspace_rays must be >= 0");
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(MCPT_ERR_ARG, "mcpt_baked_frame_params.reserved must be 0");
    if (!img) return fail(MCPT_ERR_ARG, "null image");
    return MCPT_OK;
}

static int frame_check(const mcpt_baked_source* s, const mcpt_baked_frame_params* p, const void* img)
{
    if (const int rc = baked_source_check(s)) return rc;
    return baked_frame_args_check(p, img);
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

// the device copies of a host-pointer source among the call's: `dev` is s with the device's pointers
int baked_source_upload(const mcpt_device* d, const mcpt_baked_source& s, Staging& S, mcpt_baked_source& dev)
{
    dev = s;
    if (s.kind == MCPT_BAKED_VOLUME) {
        const size_t probes = size_t(volume_probes(*s.grid));
        if (const int rc = S.in(s.sh27, probes * MCPT_SH_N * 3, "the volume's coefficients", dev.sh27)) return rc;
        if (const int rc = S.in(s.valid, probes, "the volume's mask", dev.valid)) return rc;
        const size_t bins = s.moments ? size_t(s.visibility->res) * size_t(s.visibility->res) : 0;
        if (const int rc = S.in(s.moments, probes * bins * 2, "the volume's moments", dev.moments)) return rc;
    } else {
        const size_t texels = size_t(s.width) * size_t(s.height);
        if (s.uv6)
            if (const int rc = lightmap_chart_check(s.uv6, d->ds.t)) return rc;
        if (const int rc = S.in(s.uv6, size_t(d->ds.t) * 6, "the chart", dev.uv6)) return rc;
        if (const int rc = S.in(s.irradiance3, texels * 3, "the irradiance map", dev.irradiance3)) return rc;
        if (const int rc = S.in(s.owner, texels, "the owner map", dev.owner)) return rc;
    }
    return MCPT_OK;
}

// the workspace for chunks of `rays` rays of a call on st, once the call before this one has left it (spec: a specular frame's word per ray)
static int baked_workspace(mcpt_device* d, int64_t rays, bool own_rays, bool samples, bool spec, hipStream_t st, Lease& l)
{
    if (const int rc = lease(d->baked, st, l)) return rc;
    mcpt_device::Baked& w = *d->baked;
    if (const int rc = hit_work_grow(w, rays, int64_t(1) << 40, "baked", own_rays)) return rc;
    const size_t sr = size_t(rays);
    if (samples) {
        if (const int rc = grow(w.rad, sr * 3, "the baked samples' radiance")) return rc;
        if (const int rc = grow(w.kind, sr, "the baked samples' kinds")) return rc;
        if (const int rc = grow(w.lit, sr, "the baked samples' lookups")) return rc;
    }
    if (spec)
        if (const int rc = grow(w.slit, sr, "the baked samples' specular lookups")) return rc;
    return MCPT_OK;
}

// the specular outputs of rays first .. of a call
static BakedSpecOut spec_outputs_at(const BakedSpecOut& o, int64_t first)
{
    BakedSpecOut r{};
    r.spec3 = o.spec3 ? o.spec3 + first * 3 : nullptr;
    r.ks3 = o.ks3 ? o.ks3 + first * 3 : nullptr;
    r.r3 = o.r3 ? o.r3 + first * 3 : nullptr;
    r.ns = o.ns ? o.ns + first : nullptr;
    r.slit = o.slit ? o.slit + first : nullptr;
    return r;
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
// statistics.  spec (may be null): the specular pass after every chunk's shading (mcpt.h: baked specular); without it the launches are the
// plain call's.
int baked_radiance_device(mcpt_device* d, const mcpt_baked_source& s, const double* d_rays6, int64_t n, int32_t flags, const mcpt_baked_outputs& o,
                          const BakedSpecular* spec, mcpt_stats* stats, hipStream_t st)
{
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return MCPT_OK;
    if (const int rc = motion_home(d)) return rc;           // a device that holds a motion answers from key 0
    if (const int rc = geometry_gate(d)) return rc;
    const int64_t per_chunk = chunk_plan(0, 1, n);          // the workspace of a caller's rays is the default
    Lease l;
    if (const int rc = baked_workspace(d, per_chunk, false, false, false, st, l)) return rc;
    mcpt_device::Baked& w = *d->baked;
    const BakedSource B = device_source(s);
    return chunk_run(n, per_chunk, 1, l, stats, st, [&](int64_t first, int64_t count) {
        const double* rays = d_rays6 + first * 6;
        trace_leaf(d, rays, count, w.leaf.get(), w.t.get(), w.p.get(), st);
        const BakedOut at = outputs_at(o, first);
        launch_baked_shade(d->ds, B, flags, rays, w.leaf.get(), w.t.get(), w.p.get(), count, at, st);
        if (spec)
            launch_baked_specular(d->ds, spec->V, flags, rays, w.leaf.get(), w.t.get(), w.p.get(), count, at.radiance3, spec_outputs_at(spec->rays, first), st);
        return launch_result();
    });
}

// A baked frame on st, after the refusals and the gate; device pointers throughout.  spec (may be null): the specular pass between every
// chunk's shading and its fold; without it the launches are the plain call's.
int baked_frame_device(mcpt_device* d, const mcpt_baked_source& s, const mcpt_baked_frame_params& fp, double* d_img, int32_t* d_counts3, int32_t* d_lit,
                       const BakedSpecular* spec, mcpt_stats* stats, hipStream_t st)
{
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (const int rc = motion_home(d)) return rc;
    if (const int rc = geometry_gate(d)) return rc;
    const int64_t pixels = int64_t(d->width) * d->height;
    if (pixels == 0) return MCPT_OK;
    if (const int rc = ensure_pos(d, st)) return rc;
    const int G = fp.samples;
    const int flags = fp.flags;
    const int64_t per_chunk = chunk_plan(fp.workspace_rays, G, pixels);     // whole pixels
    Lease l;
    if (const int rc = baked_workspace(d, per_chunk * G, true, true, spec && spec->pixel_slit, st, l)) return rc;
    mcpt_device::Baked& w = *d->baked;
    const BakedSource B = device_source(s);
    const DLens lens = lens_for(d, d->lens);
    return chunk_run(pixels, per_chunk, G, l, stats, st, [&](int64_t first, int64_t count) {
        BakedChunk c{};
        c.first = int(first); c.n = int(count); c.G = G;
        c.rays6 = w.rays6.get(); c.leaf = w.leaf.get(); c.t = w.t.get(); c.p = w.p.get();
        const long long rays = (long long)c.n * G;
        launch_baked_camera_rays(lens, fp.seed, c, w.rays6.get(), st);
        trace_leaf(d, c.rays6, rays, w.leaf.get(), w.t.get(), w.p.get(), st);
        BakedOut o{};
        o.radiance3 = w.rad.get(); o.kind = w.kind.get(); o.lit = w.lit.get();
        launch_baked_shade(d->ds, B, flags, c.rays6, c.leaf, c.t, c.p, rays, o, st);
        if (spec) {
            BakedSpecOut so{};
            so.slit = spec->pixel_slit ? w.slit.get() : nullptr;
            launch_baked_specular(d->ds, spec->V, flags, c.rays6, c.leaf, c.t, c.p, rays, w.rad.get(), so, st);
            if (spec->pixel_slit) launch_baked_specular_count(c, w.slit.get(), spec->pixel_slit, st);
        }
        launch_baked_fold(c, w.rad.get(), w.kind.get(), w.lit.get(), d_img, d_counts3, d_lit, st);
        return launch_result();
    });
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
    if (const int rc = device_gate(d)) return rc;
    if (n == 0) return MCPT_OK;
    launch_lightmap_irradiance(width, height, d_irradiance3, d_owner, d_uv2, n, d_e3, d_taps, static_cast<hipStream_t>(stream));
    return launch_result();
}

int mcpt_lightmap_irradiance(mcpt_device* d, int32_t width, int32_t height, const double* irradiance3, const int32_t* owner, const double* uv2, int64_t n,
                             double* e3, int32_t* taps)
{
    if (const int rc = lookup_check(width, height, irradiance3, uv2, n, e3)) return rc;
    if (const int rc = lookup_uv_check(uv2, n)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (n == 0) return MCPT_OK;
    const size_t texels = size_t(width) * size_t(height), sn = size_t(n);
    Staging S(d->stream.get());
    const double *d_irr = nullptr, *d_uv = nullptr;
    const int32_t* d_owner = nullptr;
    double* d_e = nullptr;
    int32_t* d_taps = nullptr;
    if (const int rc = S.in(irradiance3, texels * 3, "the irradiance map", d_irr)) return rc;
    if (const int rc = S.in(owner, texels, "the owner map", d_owner)) return rc;
    if (const int rc = S.in(uv2, sn * 2, "the chart coordinates", d_uv)) return rc;
    if (const int rc = S.out(e3, sn * 3, "the coordinates' irradiance", d_e)) return rc;
    if (const int rc = S.out(taps, sn, "the coordinates' taps", d_taps)) return rc;
    launch_lightmap_irradiance(width, height, d_irr, d_owner, d_uv, n, d_e, d_taps, d->stream.get());
    return S.finish(launch_result());
}

int mcpt_baked_radiance_device(mcpt_device* d, const mcpt_baked_source* s, const double* d_rays6, int64_t n, int32_t flags, const mcpt_baked_outputs* o,
                               mcpt_stats* stats, void* stream)
{
    if (const int rc = radiance_check(s, d_rays6, n, flags, o)) return rc;
    if (const int rc = device_gate(d)) return rc;
    return baked_radiance_device(d, *s, d_rays6, n, flags, *o, nullptr, stats, static_cast<hipStream_t>(stream));
}

int mcpt_baked_radiance(mcpt_device* d, const mcpt_baked_source* s, const double* rays6, int64_t n, int32_t flags, const mcpt_baked_outputs* o,
                        mcpt_stats* stats)
{
    if (const int rc = radiance_check(s, rays6, n, flags, o)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    Staging S(d->stream.get());
    mcpt_baked_source src;
    if (const int rc = baked_source_upload(d, *s, S, src)) return rc;
    if (n == 0) return MCPT_OK;
    const size_t sn = size_t(n);
    const double* d_rays = nullptr;
    mcpt_baked_outputs dev{};
    if (const int rc = S.in(rays6, sn * 6, "the rays", d_rays)) return rc;
    // one device array per output the caller asks for
    if (const int rc = S.out(o->radiance3, sn * 3, "a baked output", dev.radiance3)) return rc;
    if (const int rc = S.out(o->kind, sn, "a baked output", dev.kind)) return rc;
    if (const int rc = S.out(o->face, sn, "a baked output", dev.face)) return rc;
    if (const int rc = S.out(o->q6, sn * 6, "a baked output", dev.q6)) return rc;
    if (const int rc = S.out(o->uv2, sn * 2, "a baked output", dev.uv2)) return rc;
    if (const int rc = S.out(o->kd3, sn * 3, "a baked output", dev.kd3)) return rc;
    if (const int rc = S.out(o->e3, sn * 3, "a baked output", dev.e3)) return rc;
    if (const int rc = S.out(o->lit, sn, "a baked output", dev.lit)) return rc;
    return S.finish(baked_radiance_device(d, src, d_rays, n, flags, dev, nullptr, stats, d->stream.get()));
}

int mcpt_render_baked_device(mcpt_device* d, const mcpt_baked_source* s, const mcpt_baked_frame_params* p, double* d_img, int32_t* d_counts3, int32_t* d_lit,
                             mcpt_stats* stats, void* stream)
{
    if (const int rc = frame_check(s, p, d_img)) return rc;
    if (const int rc = device_gate(d)) return rc;
    return baked_frame_device(d, *s, *p, d_img, d_counts3, d_lit, nullptr, stats, static_cast<hipStream_t>(stream));
}

int mcpt_render_baked(mcpt_device* d, const mcpt_baked_source* s, const mcpt_baked_frame_params* p, double* img, int32_t* counts3, int32_t* lit,
                      mcpt_stats* stats)
{
    if (const int rc = frame_check(s, p, img)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    Staging S(d->stream.get());
    mcpt_baked_source src;
    if (const int rc = baked_source_upload(d, *s, S, src)) return rc;
    const size_t px = size_t(d->width) * size_t(d->height);
    if (px == 0) return MCPT_OK;
    double* d_img = nullptr;
    int32_t *d_counts = nullptr, *d_lit = nullptr;
    if (const int rc = S.out(img, px * 3, "the frame", d_img)) return rc;
    if (const int rc = S.out(counts3, px * 3, "the frame's counts", d_counts)) return rc;
    if (const int rc = S.out(lit, px, "the frame's lookups", d_lit)) return rc;
    return S.finish(baked_frame_device(d, src, *p, d_img, d_counts, d_lit, nullptr, stats, d->stream.get()));
}

}  // extern "C"
