// C ABI, rendering on a device (include/mcpt.h: mcpt_render*, mcpt_device_set_lens, mcpt_sample_radiance, mcpt_camera_rays): the launch
// sequences that stand in for generateImg of the reference -- the megakernel and the wavefront integrator, with or without a lens -- and
// their statistics.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "handles.hpp"

using namespace mcpt;

int ensure_dirs(mcpt_device* d, hipStream_t st)
{
    if (!d->dirs_ready) {
        launch_primary_dirs(d->ds.cam, d->dirs.get(), st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        d->dirs_ready = true;
    }
    return MCPT_OK;
}

// ---- lenses (mcpt.h: camera lens)
int lens_check(const mcpt_lens* l)
{
    if (!l) return MCPT_OK;
    if (l->flags & ~(MCPT_LENS_JITTER | MCPT_LENS_PER_SAMPLE)) return fail(MCPT_ERR_ARG, "unknown lens flag");
    if (l->reserved != 0) return fail(MCPT_ERR_ARG, "mcpt_lens.reserved must be 0");
    if (!(std::isfinite(l->aperture) && l->aperture >= 0.0)) return fail(MCPT_ERR_ARG, "the aperture must be finite and >= 0");
    if (!std::isfinite(l->focus_distance)) return fail(MCPT_ERR_ARG, "the focus distance must be finite");
    return MCPT_OK;
}
int ensure_pos(mcpt_device* d, hipStream_t st)
{
    if (!d->pos) {
        HIP_TRY(d->pos.alloc_bytes(std::max<size_t>(size_t(d->width) * d->height * 3 * sizeof(double), 8)));
        launch_primary_pos(d->ds.cam, d->pos.get(), st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    return MCPT_OK;
}
// what the kernels need of a lens: the device's camera frame (device.cpp: create_dscene), x^ = screen_x_dir and y^ = the normalised up as
// camera_frame forms them, F / l
DLens lens_for(const mcpt_device* d, const mcpt_lens& l)
{
    DLens c{};
    const Vec3 up = normalized(d->cam_up), dir = d->cam_look_at - d->cam_eye;
    const Vec3 x = normalized(cross(dir, up));
    const double len = norm(dir);
    const double F = l.focus_distance > 0.0 ? l.focus_distance : len;
    c.pos = d->pos.get();
    for (int i = 0; i < 3; i++) { c.eye[i] = d->ds.cam.eye[i]; c.pdx[i] = d->ds.cam.pdx[i]; c.pdy[i] = d->ds.cam.pdy[i]; }
    c.xhat[0] = x.x; c.xhat[1] = x.y; c.xhat[2] = x.z;
    c.yhat[0] = up.x; c.yhat[1] = up.y; c.yhat[2] = up.z;
    c.aperture = l.aperture;
    c.focus_scale = F / len;
    c.flags = l.flags;
    return c;
}

// the next unused start/stop pair of a pool, created on first use
static int next_pair(std::vector<EventPair>& pool, size_t& used, EventPair*& out)
{
    if (used == pool.size()) {
        EventPair q;
        HIP_TRY(create(q.first, hipEventCreate));
        HIP_TRY(create(q.second, hipEventCreate));
        pool.push_back(std::move(q));
    }
    out = &pool[used++];
    return MCPT_OK;
}

// ------------------------------------------------------------------------------------------------ integrator
static int prepare_partition(mcpt_device* d, const mcpt_render_params* p, hipStream_t st)
{
    TileShape t;
    if (const int rc = tile_shape(p, t)) return rc;
    const int key[4] = {t.tw, t.th, t.rank, t.world};
    if (std::memcmp(key, d->part_key, sizeof key) == 0 && d->pixels) return MCPT_OK;
    std::vector<int32_t> v;
    if (const int rc = owned_pixels(d->width, d->height, p, v)) return rc;
    if (d->pixels) HIP_TRY(hipDeviceSynchronize());       // a frame of the previous partition may still be in flight (MCPT_RENDER_KEEP_STATS / PIPELINE)
    HIP_TRY(d->pixels.upload(v));                          // (blocking copy: v is pageable)
    d->n_pixels = int64_t(v.size());
    std::memcpy(d->part_key, key, sizeof key);
    return MCPT_OK;
}

// Where the camera samples of a render call come from.  The per-pixel route: neither (the pixel's shared primary hit).  The per-sample
// route: an active lens (a camera ray per sample, camera.hip) or a query list (the caller's ray per sample, query.hip) -- one source
// pass, the same trace and logic launches after it, and the source's own fold.
struct SampleSource {
    const DLens* lens = nullptr;
    const DQuery* query = nullptr;
    bool per_sample() const { return lens || query; }
};

// (S.env active: a missed pixel -- or camera ray -- folds the environment's radiance; d_dirs: the pinhole's primary directions; seed: the
// call's, from which a probe list's fold draws its samples' directions again)
static void fold_range(mcpt_device::FrameSlot& f, const SampleRange& r, const PixelList& L, int first, int n_slots, double* d_img, bool lensed, const DScene& S,
                       const double* d_dirs, unsigned long long seed, hipStream_t st)
{
    if (r.query && r.query->kind == MCPT_QUERY_KIND_SPHERE)
        launch_query_fold_sh(*r.query, seed, L.pixels, f.rad.get(), f.cam_hit.get(), first, n_slots, r.n, r.k0, env_on(S.env), st);
    else if (r.query && r.moments) launch_query_fold_moments(*r.moments, f.rad.get(), f.cam_hit.get(), first, n_slots, r.n, env_on(S.env), st);
    else if (r.query) launch_query_fold(*r.query, f.rad.get(), f.cam_hit.get(), first, n_slots, r.n, env_on(S.env), st);
    else if (r.motion && !lensed) launch_fold_motion(f.rad.get(), L.pixels, f.hits.get(), first, n_slots, r.n, r.k0, r.N, d_img, r.mom, r.hit, S.env, d_dirs, st);
    else if (lensed) launch_fold_lens(f.rad.get(), f.cam_hit.get(), L.pixels, first, n_slots, r.n, r.k0, r.N, d_img, r.mom, r.hit, r.hitcnt, env_on(S.env), st);
    else if (r.mom) launch_fold_progressive(f.rad.get(), L.pixels, f.hits.get(), first, n_slots, r.n, r.k0, r.N, d_img, r.mom, r.hit, S.env, d_dirs, st);
    else launch_fold_samples(f.rad.get(), L.pixels, f.hits.get(), first, n_slots, r.n, d_img, S.env, d_dirs, st);
}

// megakernel path: one lane per camera sample, the whole path in one kernel (kept for A/B runs and as a second
// implementation the wavefront path is checked against)
static int render_megakernel(mcpt_device* d, const DScene& S, mcpt_device::FrameSlot& f, const SampleRange& r, const PixelList& L, const mcpt_render_params* p,
                             double* d_img, bool timed, const SampleSource& src, hipStream_t st, double& ms_trace, int& launches)
{
    const int64_t npx = L.n;
    const int spp = r.n;
    const bool per_sample = src.per_sample();
    const size_t per_pixel = size_t(spp) * 3 * sizeof(double) + (per_sample ? size_t(spp) : 0);   // (+ the hit flag of every sample under a lens)
    int64_t chunk = int64_t(std::max<size_t>(d->sample_budget_bytes / per_pixel, 64));
    chunk = std::min<int64_t>(chunk, npx);
    HIP_TRY(f.rad.grow_bytes(size_t(chunk) * per_pixel));
    if (per_sample) HIP_TRY(f.cam_hit.grow(size_t(chunk * spp)));
    for (int64_t first = 0; first < npx; first += chunk) {
        const int n_slots = int(std::min<int64_t>(chunk, npx - first));
        if (timed) HIP_TRY(hipEventRecord(d->ev[2].get(), st));
        if (src.query) launch_query_samples(S, *src.query, p->seed, L.pixels, int(first), n_slots, spp, r.k0, f.rad.get(), f.cam_hit.get(), f.ctr.get(), st);
        else if (per_sample) launch_shade_samples_lens(S, *src.lens, p->seed, L.pixels, int(first), n_slots, spp, r.k0, f.rad.get(), f.cam_hit.get(), f.ctr.get(), st);
        else launch_shade_samples(S, p->seed, d->dirs.get(), L.pixels, f.hits.get(), int(first), n_slots, spp, r.k0, f.rad.get(), f.ctr.get(), st);
        HIP_TRY(hipGetLastError());
        if (timed) {
            HIP_TRY(hipEventRecord(d->ev[3].get(), st));
            HIP_TRY(hipEventSynchronize(d->ev[3].get()));
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, d->ev[2].get(), d->ev[3].get()));
            ms_trace += ms;
        }
        launches++;
        fold_range(f, r, L, int(first), n_slots, d_img, per_sample, S, d->dirs.get(), p->seed, st);
        HIP_TRY(hipGetLastError());
    }
    return MCPT_OK;
}

// wavefront path (wavefront.hpp): per chunk, lockstep iterations of logic + trace over compacted path state in HBM.
// timed: event pairs around the trace launches, summed here (one stream synchronisation at the end); keep: the pairs are recorded
// and left in d->ev_pool for mcpt_device_collect_stats -- the frame ends without the host waiting for it.
// src (a lens or a query list): the per-sample route -- per chunk a source pass (the camera, or the caller's ray, as vertex -1 of every
// sample) and a trace launch of its rays, then the logic passes from depth 0 on, every vertex in the path state (WfArgs::hits == null)
static int render_wavefront(mcpt_device* d, const DScene& S, mcpt_device::FrameSlot& f, const SampleRange& r, const PixelList& L, const mcpt_render_params* p,
                            double* d_img, bool timed, bool keep, const SampleSource& src, hipStream_t st, double& ms_trace, int& launches)
{
    const int64_t npx = L.n;
    const int spp = r.n;
    const bool per_sample = src.per_sample();
    // WfArgs::nl: shadow planes -- one per light and one for an active environment (its draws use Philox block num_lights + 2)
    // (MCPT_LIGHTS_ONE: one plane for the picked light, whatever the scene's count -- which stays the Philox block base, S.num_lights)
    const int nl = (pick_on(S.pick) ? 1 : S.num_lights) + (env_on(S.env) ? 1 : 0);
    const bool fast = d->trace_mode == MCPT_TRACE_FAST;
    const size_t bpp = wf_bytes_per_path(nl);
    // chunk: as many pixels as the workspace budget holds paths for (every pixel may hit)
    const size_t overhead = 64 * 1024;
    // Fewer, larger chunks are cheaper (every chunk ends in a tail of small launches): by default a frame slot may use half of
    // the HBM that is free (a third when two frames are pipelined), which holds a whole 1280x720 SPP-256 frame (83 GB) on a
    // 288-GB device.
    size_t budget = d->wf_budget_bytes;
    if (!budget) {
        if (!d->wf_auto_budget) {
            size_t free_b = 0, total_b = 0;
            HIP_TRY(hipMemGetInfo(&free_b, &total_b));
            size_t mine = 0;
            for (const auto& q : d->slot) mine += q.wf_ws.bytes() + q.rad.bytes();
            d->wf_auto_budget = std::max<size_t>((free_b + mine) / (d->pipelined ? 3 : 2), size_t(1) << 30);
        }
        budget = d->wf_auto_budget;
    }
    int64_t cap = int64_t((budget - overhead) / (bpp + 24 + (per_sample ? 1 : 0)));      // + 24 B radiance per sample (+ its hit flag under a lens)
    cap = std::min<int64_t>(cap, npx * int64_t(spp));
    cap = std::min<int64_t>(cap, (int64_t(1) << 31) - 4096);                 // 32-bit compaction counter / sample ids
    int64_t chunk_slots = std::max<int64_t>(cap / spp, 1);
    chunk_slots = std::min<int64_t>(chunk_slots, npx);
    cap = chunk_slots * spp;
    const size_t ws_need = size_t(cap) * bpp + overhead;
    HIP_TRY(f.wf_ws.grow_bytes(ws_need));
    HIP_TRY(f.rad.grow_bytes(size_t(cap) * 3 * sizeof(double)));
    if (per_sample) {
        HIP_TRY(f.cam_hit.grow(size_t(cap)));
    } else {
        HIP_TRY(f.hit_slots.grow(size_t(chunk_slots)));
        HIP_TRY(f.surf.grow(size_t(chunk_slots)));
        HIP_TRY(f.alive_base.grow(size_t(chunk_slots / 64 + 2)));
    }
    int rc = MCPT_OK;
    WfArgs a{};
    WfState A, B;
    if (!wf_carve(f.wf_ws.get(), f.wf_ws.bytes(), cap, nl, A, B, a.rays)) return fail(MCPT_ERR_NOMEM, "wavefront workspace too small");
    // the pool form of the finishing pass keeps nl + 1 rays per path: its area was sized for the scene's lights when the device was made
    char* path_area = f.path_area.get();
    if (nl != S.num_lights && d->cfg.finish_pool) {
        const size_t need = finish_pool_bytes(d->cfg.cus, nl);
        if (!need) path_area = nullptr;
        else { HIP_TRY(f.path_area.grow_bytes(need)); path_area = f.path_area.get(); }
    }
    a.cap = cap; a.nl = nl; a.spp = spp; a.sample_base = r.k0; a.seed = p->seed; a.pixels = L.pixels; a.hit_slots = f.hit_slots.get(); a.surf = f.surf.get(); a.alive_base = f.alive_base.get();
    a.hits = f.hits.get(); a.dirs = d->dirs.get(); a.rad = f.rad.get(); a.counts = f.wf_counts.get(); a.ctr = f.ctr.get(); a.tris = d->tris.get();
    a.materials = d->materials.get(); a.queue = fast ? f.queue.get() : nullptr;
    a.finish_below = fast ? unsigned(std::min<long long>(std::max<long long>(d->finish_threshold, 0), 1ll << 30)) : 0u;
    if (per_sample) { a.hits = nullptr; a.cam_hit = f.cam_hit.get(); }
    // Iterations are enqueued without waiting for their counts: every kernel reads its input count from the device slot the
    // previous one wrote.  The host looks at a count only every few iterations (to stop, and to size the next grids).
    const size_t ev_first = d->ev_used;
    const int kSyncEvery = 4;
    for (int64_t first = 0; first < npx; first += chunk_slots) {
        const int n_slots = int(std::min<int64_t>(chunk_slots, npx - first));
        HIP_TRY(hipMemsetAsync(f.wf_counts.get(), 0, sizeof(WfCounts) * MCPT_WF_COUNT_SLOTS, st));
        long long n_upper = (long long)n_slots * spp;        // upper bound of the live paths, refined at every look
        double n_grid = double(n_upper);                     // grid-sizing estimate between looks (kernels stride, any grid is correct)
        a.first_slot = int(first);
        a.in = A; a.out = B;
        a.counts_in = &f.wf_counts[0];
        if (per_sample) {
            // the camera as vertex -1: its state into a.out, the count into slot 0, its rays traced as a bounce (depth -1: from a.out.p)
            WfArgs ac = a;
            ac.depth = -1; ac.counts = &f.wf_counts[0]; ac.count_mul = 1u; ac.finish_below = 0u;
            if (src.query) launch_query_pass(*src.query, ac, n_upper, st);
            else launch_camera_pass(*src.lens, ac, n_upper, st);
            HIP_TRY(hipGetLastError());
            ac.nl = 0;          // the trace launch sees the bounce slot only (l == nl): no empty shadow-ray slots to walk past
            EventPair* pr = nullptr;
            if (timed || keep) { if ((rc = next_pair(d->ev_pool, d->ev_used, pr))) return rc; HIP_TRY(hipEventRecord(pr->first.get(), st)); }
            launch_wf_trace(S, ac, n_upper, fast, f.queue.get(), f.slow_list.get(), d->slow_cap, st, d->cfg);
            HIP_TRY(hipGetLastError());
            if (timed || keep) HIP_TRY(hipEventRecord(pr->second.get(), st));
            launches++;
            std::swap(a.in, a.out);
        } else {
            launch_hit_slots(f.hits.get(), int(first), n_slots, f.hit_slots.get(), &f.wf_counts[0].n_next, st);
            HIP_TRY(hipGetLastError());
            launch_primary_surface(S, a, f.surf.get(), f.alive_base.get(), &f.wf_counts[0].shaded_pixels, n_slots, st);      // what the samples of a pixel share at their first vertex
            HIP_TRY(hipGetLastError());
        }
        for (int depth = 0; depth < MCPT_MAX_DEPTH && n_upper > 0; depth++) {
            a.depth = depth;
            a.counts_in = &f.wf_counts[depth]; a.count_mul = depth == 0 && !per_sample ? unsigned(spp) : 1u;
            a.counts = &f.wf_counts[depth + 1];
            const long long n_launch = std::max<long long>(1, (long long)n_grid);
            // the per-sample route's depth 0 resolves the camera rays: nothing went to the finishing kernel before it, and its pool form
            // (which reads a pixel's PrimaryHit at depth 0) does not adopt its paths
            const bool cam0 = per_sample && depth == 0;
            char* const area = cam0 ? nullptr : path_area;
            if (cam0) { WfArgs al = a; al.finish_below = 0u; launch_wf_logic(S, al, n_launch, false, st, d->cfg); }
            else launch_wf_logic(S, a, n_launch, depth == 0, st, d->cfg);
            HIP_TRY(hipGetLastError());
            // The host looks at this pass's count every few iterations, and at every iteration once the hand-over to the finishing
            // kernel is near.  The look waits for this logic pass only (event + side stream): when it finds the hand-over, the
            // finishing kernel is launched and the call returns while it runs -- the next frame's head can overlap it.
            const bool look = (depth + 1) % kSyncEvery == 0 || (a.finish_below && n_grid * 0.6 <= 6.0 * double(a.finish_below));
            if (look) {
                HIP_TRY(hipEventRecord(d->look_ev.get(), st));
                HIP_TRY(hipStreamWaitEvent(d->look_stream.get(), d->look_ev.get(), 0));
                HIP_TRY(hipMemcpyAsync(d->h_look.get(), &f.wf_counts[depth + 1].n_next, sizeof(unsigned int), hipMemcpyDeviceToHost, d->look_stream.get()));
                HIP_TRY(hipStreamSynchronize(d->look_stream.get()));
                const unsigned int n_now = d->h_look[0];
                if (n_now <= a.finish_below) {
                    if (n_now > 0) { launch_wf_finish(S, a, (long long)n_now, st, d->cfg, area, f.slow_list.get(), d->slow_cap); HIP_TRY(hipGetLastError()); }
                    n_upper = 0;
                    break;
                }
                n_upper = n_now;
                n_grid = double(n_now);
            } else if (a.finish_below) {
                // few paths left (decided on the device from this pass's count): one lane per path runs them to the end
                launch_wf_finish(S, a, std::min<long long>(n_launch, (long long)a.finish_below), st, d->cfg, area, f.slow_list.get(), d->slow_cap);
                HIP_TRY(hipGetLastError());
            }
            const long long n_trace = look ? (long long)n_grid : n_launch;
            EventPair* pr = nullptr;
            if (timed || keep) { if ((rc = next_pair(d->ev_pool, d->ev_used, pr))) return rc; HIP_TRY(hipEventRecord(pr->first.get(), st)); }
            launch_wf_trace(S, a, n_trace, fast, f.queue.get(), f.slow_list.get(), d->slow_cap, st, d->cfg);
            HIP_TRY(hipGetLastError());
            if (timed || keep) HIP_TRY(hipEventRecord(pr->second.get(), st));
            launches++;
            std::swap(a.in, a.out);
            if (!look) n_grid *= 0.75;   // paths die at >= 40 % per bounce (Russian roulette 0.6)
        }
        // paths still alive at the depth cap cannot exist: logic(MAX_DEPTH-1) emits no bounce ray; a last logic pass resolves them
        if (n_upper > 0) {
            a.depth = MCPT_MAX_DEPTH;
            a.counts_in = &f.wf_counts[MCPT_MAX_DEPTH]; a.count_mul = 1u; a.counts = &f.wf_counts[MCPT_MAX_DEPTH + 1];
            launch_wf_logic(S, a, n_upper, false, st, d->cfg);
            HIP_TRY(hipGetLastError());
        }
        fold_range(f, r, L, int(first), n_slots, d_img, per_sample, S, d->dirs.get(), p->seed, st);
        HIP_TRY(hipGetLastError());
    }
    if (timed && !keep) {
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t i = ev_first; i < d->ev_used; i++) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, d->ev_pool[i].first.get(), d->ev_pool[i].second.get()));
            ms_trace += ms;
        }
        d->ev_used = ev_first;
    }
    return MCPT_OK;
}

int render_device_impl(mcpt_device* d, const SampleRange& r, const PixelList& L, const mcpt_render_params* p, double* d_img, mcpt_stats* stats,
                       hipStream_t st, int& slot_used)
{
    const bool keep = (p->flags & MCPT_RENDER_KEEP_STATS) != 0 && !(p->flags & MCPT_RENDER_MEGAKERNEL);
    const bool timed = stats != nullptr && !keep;
    // frame slot: consecutive pipelined frames alternate; a slot's previous frame (possibly on another stream) must be over
    if ((p->flags & MCPT_RENDER_PIPELINE) && !d->pipelined) {
        HIP_TRY(hipDeviceSynchronize());
        d->pipelined = true; d->wf_auto_budget = 0;                  // the budget now has to hold two frames
        for (auto& q : d->slot) q.wf_ws.reset();
    }
    const int si = (p->flags & MCPT_RENDER_PIPELINE) ? (d->next_slot ^= 1) : 0;
    slot_used = si;
    mcpt_device::FrameSlot& f = d->slot[si];
    if (f.used) HIP_TRY(hipStreamWaitEvent(st, f.done.get(), 0));
    int rc = r.query ? MCPT_OK : ensure_dirs(d, st);        // (nothing of the frame enters a query)
    if (rc) return rc;
    const bool with_lens = !r.query && r.lens && lens_active(*r.lens);
    const bool lensed = with_lens || r.query;           // the per-sample route
    if (with_lens && (rc = ensure_pos(d, st))) return rc;
    const DLens dl = with_lens ? lens_for(d, *r.lens) : DLens{};
    const SampleSource src{with_lens ? &dl : nullptr, r.query};
    DScene S = d->ds;                                   // the scene with the environment of the call
    S.env = r.env ? r.env->denv : DEnv{};
    const int64_t npx = L.n;
    if (npx == 0) return MCPT_OK;
    const uint64_t primary_rays = uint64_t(npx) * (lensed ? uint64_t(r.n) : 1u);
    if (!r.query) HIP_TRY(f.hits.grow(size_t(npx)));        // (a query's slots are no pixels: nothing of it has a primary hit record)
    if (!keep || !f.keeping) HIP_TRY(hipMemsetAsync(f.ctr.get(), 0, sizeof(DCounters), st));    // kept statistics accumulate until they are collected
    f.keeping = keep;
    EventPair* fe = nullptr;
    if (keep) {
        if ((rc = next_pair(d->frame_ev, d->frame_ev_used, fe))) return rc;
        HIP_TRY(hipEventRecord(fe->first.get(), st));
    } else HIP_TRY(hipEventRecord(d->ev[0].get(), st));
    if (!lensed) {          // (a lens traces its camera rays per sample, in the render path)
        launch_primary_hits(d->ds, d->trace_mode == MCPT_TRACE_FAST, d->dirs.get(), L.pixels, int(npx), f.hits.get(), f.ctr.get(), f.queue.get(), f.slow_list.get(), d->slow_cap, st, d->cfg);
        HIP_TRY(hipGetLastError());
    }
    double ms_trace = 0;
    int launches = 0;
    if (p->flags & MCPT_RENDER_MEGAKERNEL) rc = render_megakernel(d, S, f, r, L, p, d_img, timed, src, st, ms_trace, launches);
    else rc = render_wavefront(d, S, f, r, L, p, d_img, timed, keep, src, st, ms_trace, launches);
    if (rc) return rc;
    if (keep) {
        HIP_TRY(hipEventRecord(fe->second.get(), st));
        d->kept_samples += uint64_t(npx) * uint64_t(r.n); d->kept_primary += primary_rays; d->kept_launches += launches;
    } else HIP_TRY(hipEventRecord(d->ev[1].get(), st));
    HIP_TRY(hipEventRecord(f.done.get(), st));
    f.used = true;
    if (timed) {
        DCounters c{};
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemcpy(&c, f.ctr.get(), sizeof c, hipMemcpyDeviceToHost));
        counters_to_stats(c, stats, d->knobs.print_diag != 0);
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, d->ev[0].get(), d->ev[1].get()));
        stats->ms_total = ms; stats->ms_trace = ms_trace; stats->launches = launches;
        stats->samples = uint64_t(npx) * uint64_t(r.n);         // camera samples covered (a primary miss is a finished sample)
        stats->rays_primary = primary_rays;
    }
    return MCPT_OK;
}

// The (pixel, sample) queries: n pairs (pix[i], k[i]) -> per doubles each in out.  prepare(d, st) makes what the launch reads, on the
// library stream; launch(d_pix, d_k, d_out, st) enqueues the kernel; the call waits for it and reads the answers back.
template <class Prepare, class Launch>
static int pair_call(mcpt_device* d, const int32_t* pix, const int32_t* k, int64_t n, double* out, int per, Prepare prepare, Launch launch)
{
    if (n == 0) return MCPT_OK;
    for (int64_t i = 0; i < n; i++)
        if (pix[i] < 0 || pix[i] >= d->width * d->height) return fail(MCPT_ERR_ARG, "pixel index out of range");
    HIP_TRY(hipSetDevice(d->ordinal));
    hipStream_t st = d->stream.get();
    if (const int rc = prepare(d, st)) return rc;
    Staging S(st);
    const int32_t *d_pix = nullptr, *d_k = nullptr;
    double* d_out = nullptr;
    if (const int rc = S.in(pix, size_t(n), "the pixels", d_pix)) return rc;
    if (const int rc = S.in(k, size_t(n), "the samples", d_k)) return rc;
    if (const int rc = S.out(out, size_t(n) * per, "the pairs' answers", d_out)) return rc;
    const int rc = launch(d_pix, d_k, d_out, st);
    return S.finish(rc == MCPT_OK ? launch_result() : rc);
}

// The shutter frame of a device with a motion (mcpt.h: motion blur): the frame's samples in the shutter's steps, each piece a progressive
// pass on the step's geometry and camera that continues the fold in d_img; the moments it needs beside are the motion's own.
static int render_motion_frame(mcpt_device* d, const mcpt_render_params* p, double* d_img, mcpt_stats* stats, hipStream_t st)
{
    mcpt_device::Motion& m = *d->motion;
    if (p->flags & MCPT_RENDER_PIPELINE) return fail(MCPT_ERR_ARG, "a motion frame takes no MCPT_RENDER_PIPELINE: its steps are joined by synchronous updates");
    if (m.shutter.steps > p->spp) return fail(MCPT_ERR_ARG, "the shutter has more steps than the frame has samples per pixel");
    const size_t px = size_t(d->width) * d->height;
    const bool lensed = lens_active(d->lens);
    if (!m.mom) HIP_TRY(m.mom.alloc(std::max<size_t>(px * 6, 1)));
    if (!m.hit) HIP_TRY(m.hit.alloc(std::max<size_t>(px, 8)));
    if (lensed && !m.hitcnt) HIP_TRY(m.hitcnt.alloc(std::max<size_t>(px, 2)));
    if (const int rc = prepare_partition(d, p, st)) return rc;
    const size_t ev_used0 = d->ev_used, frame_ev_used0 = d->frame_ev_used;
    int slot_used = -1;
    const int rc = motion_passes(d, 0, p->spp, p->spp, st, [&](int lo, int cnt) {
        const SampleRange r{lo, cnt, p->spp, m.mom.get(), m.hit.get(), &d->lens, lensed ? m.hitcnt.get() : nullptr, d->env.get(), true};
        mcpt_stats piece{};
        const int prc = render_device_impl(d, r, PixelList{d->pixels.get(), d->n_pixels}, p, d_img, stats ? &piece : nullptr, st, slot_used);
        if (prc != MCPT_OK && slot_used >= 0) d->slot[slot_used].keeping = false;      // its counters hold part of a frame
        if (prc == MCPT_OK && stats) add_piece(*stats, piece);
        return prc;
    });
    if (rc != MCPT_OK) { d->ev_used = ev_used0; d->frame_ev_used = frame_ev_used0; }
    return rc;
}

extern "C" {

int mcpt_render_device(mcpt_device* d, const mcpt_render_params* p, double* d_img, mcpt_stats* stats, void* stream)
{
    if (!d || !p || !d_img || p->spp <= 0) return fail(MCPT_ERR_ARG, "bad argument");
    if (const int rc = geometry_gate(d)) return rc;
    HIP_TRY(hipSetDevice(d->ordinal));
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (d->motion) return render_motion_frame(d, p, d_img, stats, static_cast<hipStream_t>(stream));
    // a frame that fails half-way must not leave half-recorded event pairs behind: mcpt_device_collect_stats would trip over them
    const size_t ev_used0 = d->ev_used, frame_ev_used0 = d->frame_ev_used;
    int slot_used = -1;
    const SampleRange whole{0, p->spp, p->spp, nullptr, nullptr, &d->lens, nullptr, d->env.get()};
    int rc = prepare_partition(d, p, static_cast<hipStream_t>(stream));
    if (rc == MCPT_OK) rc = render_device_impl(d, whole, PixelList{d->pixels.get(), d->n_pixels}, p, d_img, stats, static_cast<hipStream_t>(stream), slot_used);
    if (rc != MCPT_OK) {
        d->ev_used = ev_used0; d->frame_ev_used = frame_ev_used0;
        if (slot_used >= 0) d->slot[slot_used].keeping = false;      // its counters hold part of a frame: cleared by the next one
    }
    return rc;
}

// Statistics of every MCPT_RENDER_KEEP_STATS frame since the last call: waits for those frames, sums the device counters of both
// frame slots, the event pairs around every k_wf_trace launch (ms_trace) and around every frame (ms_total = sum of frame times;
// pipelined frames overlap, so this can exceed the wall time), then starts over.
int mcpt_device_collect_stats(mcpt_device* d, mcpt_stats* stats)
{
    if (!d || !stats) return fail(MCPT_ERR_ARG, "null argument");
    std::memset(stats, 0, sizeof *stats);
    HIP_TRY(hipSetDevice(d->ordinal));
    HIP_TRY(hipDeviceSynchronize());
    DCounters sum{};
    for (auto& f : d->slot) {
        DCounters c{};
        HIP_TRY(hipMemcpy(&c, f.ctr.get(), sizeof c, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(f.ctr.get(), 0, sizeof(DCounters)));
        unsigned long long* a = reinterpret_cast<unsigned long long*>(&sum);
        const unsigned long long* b = reinterpret_cast<const unsigned long long*>(&c);
        for (size_t i = 0; i < sizeof(DCounters) / sizeof(unsigned long long); i++) a[i] += b[i];
        sum.max_depth = std::max(sum.max_depth - c.max_depth, c.max_depth);      // a maximum, not a sum
    }
    counters_to_stats(sum, stats, d->knobs.print_diag != 0);
    // the bookkeeping starts over whatever the queries say: a pair that cannot be read is left out and reported
    hipError_t bad = hipSuccess;
    for (size_t i = 0; i < d->ev_used; i++) {
        float ms = 0;
        const hipError_t e = hipEventElapsedTime(&ms, d->ev_pool[i].first.get(), d->ev_pool[i].second.get());
        if (e == hipSuccess) stats->ms_trace += ms; else bad = e;
    }
    for (size_t i = 0; i < d->frame_ev_used; i++) {
        float ms = 0;
        const hipError_t e = hipEventElapsedTime(&ms, d->frame_ev[i].first.get(), d->frame_ev[i].second.get());
        if (e == hipSuccess) stats->ms_total += ms; else bad = e;
    }
    stats->launches = d->kept_launches; stats->samples = d->kept_samples; stats->rays_primary = d->kept_primary;
    d->ev_used = 0; d->frame_ev_used = 0; d->kept_launches = 0; d->kept_samples = 0; d->kept_primary = 0;
    for (auto& f : d->slot) f.keeping = false;
    if (bad != hipSuccess) { (void)hipGetLastError(); return fail(MCPT_ERR_HIP, std::string("an event pair of a kept frame could not be read: ") + hipGetErrorString(bad)); }
    return MCPT_OK;
}

int mcpt_render(mcpt_device* d, const mcpt_render_params* p, double* img, mcpt_stats* stats)
{
    if (!d || !p || !img) return fail(MCPT_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(d->ordinal));
    // The caller's frame goes in and comes back: pixels this rank does not own keep the caller's values.
    Staging S(d->stream.get());
    double* d_img = nullptr;
    if (const int rc = S.inout(img, size_t(d->width) * d->height * 3, "the frame", d_img)) return rc;
    return S.finish(mcpt_render_device(d, p, d_img, stats, d->stream.get()));
}

int mcpt_sample_radiance(mcpt_device* d, uint64_t seed, const int32_t* pix, const int32_t* k, int64_t n, double* rgb)
{
    if (!d || !pix || !k || !rgb || n < 0) return fail(MCPT_ERR_ARG, "bad argument");
    if (const int rc = motion_home(d)) return rc;
    if (const int rc = geometry_gate(d)) return rc;
    return pair_call(d, pix, k, n, rgb, 3, ensure_dirs, [&](const int32_t* d_pix, const int32_t* d_k, double* d_rgb, hipStream_t st) {
        if (lens_active(d->lens)) {
            if (const int rc = ensure_pos(d, st)) return rc;
            launch_sample_radiance_lens(d->ds, lens_for(d, d->lens), seed, d_pix, d_k, n, d_rgb, d->aux_ctr.get(), st);
        } else launch_sample_radiance(d->ds, seed, d->dirs.get(), d_pix, d_k, n, d_rgb, d->aux_ctr.get(), st);
        return MCPT_OK;
    });
}

int mcpt_device_set_lens(mcpt_device* d, const mcpt_lens* l)
{
    if (int rc = lens_check(l)) return rc;
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    d->lens = l ? *l : mcpt_lens{};
    return MCPT_OK;
}

int mcpt_device_get_lens(const mcpt_device* d, mcpt_lens* out)
{
    if (!out) return fail(MCPT_ERR_ARG, "null argument");
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    *out = d->lens;
    return MCPT_OK;
}

int mcpt_camera_rays(mcpt_device* d, uint64_t seed, const int32_t* pix, const int32_t* k, int64_t n, double* rays6)
{
    if (!pix || !k || !rays6 || n < 0) return fail(MCPT_ERR_ARG, "bad argument");
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    return pair_call(d, pix, k, n, rays6, 6, ensure_pos, [&](const int32_t* d_pix, const int32_t* d_k, double* d_rays, hipStream_t st) {
        launch_camera_rays(lens_for(d, d->lens), seed, d_pix, d_k, n, d_rays, st);
        return MCPT_OK;
    });
}

}  // extern "C"
