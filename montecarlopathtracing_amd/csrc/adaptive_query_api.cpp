// C ABI, adaptive radiance queries (include/mcpt.h: mcpt_query_radiance_adaptive*, mcpt_query_pass_boundaries): mcpt_query_radiance in
// passes whose boundaries double from min_spp, every query leaving the list on its own error estimate.  A pass is an ordinary query call
// over the compact list of the active queries (render.cpp: the per-sample route, unchanged) whose fold continues the moments of the
// caller's positions; the selection is the adaptive frames' three kernels over list positions (kernels.hip, unchanged).  The host reads
// back 4 bytes per pass: the next list's length.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "handles.hpp"

using namespace mcpt;

// b_0 = min(min_spp, spp), b_{j+1} = min(2 b_j, spp) in 64 bits, up to spp itself (spp >= 1, min_spp >= 1)
static std::vector<int32_t> pass_boundaries(int32_t spp, int32_t min_spp)
{
    std::vector<int32_t> b;
    int64_t k = std::min<int64_t>(min_spp, spp);
    for (;;) {
        b.push_back(int32_t(k));
        if (k >= spp) break;
        k = std::min<int64_t>(2 * k, spp);
    }
    return b;
}

int adaptive_params_check(const mcpt_adaptive_params* ap)
{
    if (!ap) return fail(MCPT_ERR_ARG, "null adaptive parameters");
    if (!(std::isfinite(ap->rel_target) && ap->rel_target >= 0.0 && std::isfinite(ap->abs_target) && ap->abs_target >= 0.0))
        return fail(MCPT_ERR_ARG, "rel_target and abs_target must be finite and >= 0");
    if (ap->min_spp < 2) return fail(MCPT_ERR_ARG, "min_spp must be >= 2 (a standard error needs two samples)");
    if (ap->reserved != 0) return fail(MCPT_ERR_ARG, "mcpt_adaptive_params.reserved must be 0");
    return MCPT_OK;
}

// the workspace of a list of n queries on d for a call on st, once the call before this one has left it
static int ensure_work(mcpt_device* d, size_t n, hipStream_t st, Lease& l)
{
    const auto words = [](mcpt_device::AdaptiveQuery& w) -> int {
        HIP_TRY(w.h_total.alloc(1));
        HIP_TRY(w.total.alloc(1));
        return MCPT_OK;
    };
    if (const int rc = lease(d->aq, st, l, words)) return rc;
    mcpt_device::AdaptiveQuery& w = *d->aq;
    const size_t blocks = size_t((n + 255) / 256);
    const char* what = "the adaptive query's workspace";
    if (const int rc = grow(w.mom, n * 6, what)) return rc;
    if (const int rc = grow(w.hitcnt, n, what)) return rc;
    if (const int rc = grow(w.cnt, n, what)) return rc;
    if (const int rc = grow(w.sel[0], n, what)) return rc;
    if (const int rc = grow(w.sel[1], n, what)) return rc;
    if (const int rc = grow(w.ones, n, what)) return rc;
    if (const int rc = grow(w.masks, blocks * 4, what)) return rc;
    if (const int rc = grow(w.block_counts, blocks, what)) return rc;
    return grow(w.block_offsets, blocks, what);
}

// the passes and the finishing kernel on st; the gates have been passed and the workspace is the call's
static int run_passes(mcpt_device* d, const DQuery& q, const int32_t* d_ids, int64_t n, int32_t spp, int32_t sample_base, uint64_t seed, int32_t flags,
                      const mcpt_adaptive_params& ap, int32_t* d_counts, mcpt_stats* stats, hipStream_t st)
{
    mcpt_device::AdaptiveQuery& w = *d->aq;
    const size_t sn = size_t(n);
    const int32_t min_spp = std::min(ap.min_spp, spp);
    const double rel2 = ap.rel_target * ap.rel_target, abs2 = ap.abs_target * ap.abs_target;
    const std::vector<int32_t> bounds = pass_boundaries(spp, min_spp);
    HIP_TRY(hipMemsetAsync(w.mom.get(), 0, sn * 6 * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(w.hitcnt.get(), 0, sn * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(w.ones.get(), 1, sn, st));
    launch_aq_iota(w.sel[0].get(), n, st);
    HIP_TRY(hipGetLastError());
    mcpt_render_params rp{};
    rp.seed = seed; rp.world = 1; rp.flags = flags;
    int cur = 0, slot_used = -1;
    int64_t active = n;
    int32_t prev = 0;
    for (size_t j = 0; j < bounds.size(); j++) {
        const int32_t k = bounds[j], cnt = k - prev;
        // the first pass's list is the caller's own; later ones are gathered from it
        const double* pq6 = q.q6;
        const int32_t* pids = d_ids;
        if (j > 0) {
            if (const int rc = grow(w.cq6, size_t(active) * 6, "the adaptive query's compact list")) return rc;
            if (const int rc = grow(w.cids, size_t(active), "the adaptive query's compact list")) return rc;
            launch_aq_gather(q.q6, d_ids, w.sel[cur].get(), active, w.cq6.get(), w.cids.get(), st);
            HIP_TRY(hipGetLastError());
            pq6 = w.cq6.get(); pids = w.cids.get();
        }
        const DQuery cq{pq6, q.kind, nullptr, nullptr, nullptr};
        const QueryMoments qm{w.mom.get(), w.hitcnt.get(), w.sel[cur].get()};
        SampleRange r{sample_base + prev, cnt, cnt, nullptr, nullptr, nullptr, nullptr, d->env.get()};
        r.query = &cq; r.moments = &qm;
        rp.spp = cnt;
        mcpt_stats piece{};
        if (const int rc = render_device_impl(d, r, PixelList{pids, active}, &rp, nullptr, stats ? &piece : nullptr, st, slot_used)) return rc;
        if (stats) add_piece(*stats, piece);
        // which queries continue, and every active query's count: decided on the device over list positions (no miss rule: the hit bytes are ones)
        launch_adaptive_select(w.sel[cur].get(), int(active), w.mom.get(), w.ones.get(), k, min_spp, rel2, abs2, w.cnt.get(), w.masks.get(),
                               w.block_counts.get(), w.block_offsets.get(), w.total.get(), w.sel[cur ^ 1].get(), st);
        HIP_TRY(hipGetLastError());
        if (j + 1 == bounds.size()) break;
        HIP_TRY(hipMemcpyAsync(w.h_total.get(), w.total.get(), sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        active = w.h_total[0];
        cur ^= 1;
        prev = k;
        if (active == 0) break;
    }
    launch_aq_finish(w.mom.get(), w.hitcnt.get(), w.cnt.get(), n, q.mean3, q.stderr3, q.hits, d_counts, st);
    HIP_TRY(hipGetLastError());
    return MCPT_OK;
}

int adaptive_query_device(mcpt_device* d, const DQuery& q, const int32_t* d_ids, int64_t n, int32_t spp, int32_t sample_base, uint64_t seed, int32_t flags,
                          const mcpt_adaptive_params& ap, int32_t* d_counts, mcpt_stats* stats, void* stream)
{
    if (const int rc = device_gate(d)) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return MCPT_OK;
    if (const int rc = motion_home(d)) return rc;           // a device that holds a motion answers from key 0
    if (const int rc = geometry_gate(d)) return rc;
    if (const int rc = wait_for_frames(d)) return rc;       // the passes use frame slot 0 and the device's look stream
    hipStream_t st = static_cast<hipStream_t>(stream);
    Lease l;
    if (const int rc = ensure_work(d, size_t(n), st, l)) return rc;
    // a call that fails half-way must not leave half-recorded event pairs behind (render.cpp: mcpt_render_device)
    const size_t ev_used0 = d->ev_used;
    const int rc = run_passes(d, q, d_ids, n, spp, sample_base, seed, flags, ap, d_counts, stats, st);
    if (rc != MCPT_OK) d->ev_used = ev_used0;
    return l.end(rc);
}

extern "C" {

int mcpt_query_pass_boundaries(int32_t spp, int32_t min_spp, int32_t* bounds, int32_t cap)
{
    if (spp < 1) return fail(MCPT_ERR_ARG, "spp must be >= 1");
    if (min_spp < 2) return fail(MCPT_ERR_ARG, "min_spp must be >= 2 (a standard error needs two samples)");
    if (cap < 0) return fail(MCPT_ERR_ARG, "cap must be >= 0");
    const std::vector<int32_t> b = pass_boundaries(spp, min_spp);
    if (bounds) {
        if (int64_t(b.size()) > cap) return fail(MCPT_ERR_ARG, "more pass boundaries (" + std::to_string(b.size()) + ") than the list holds");
        std::copy(b.begin(), b.end(), bounds);
    }
    return int(b.size());
}

int mcpt_query_radiance_adaptive_device(mcpt_device* d, const double* d_q6, const int32_t* d_ids, int64_t n, const mcpt_query_params* p,
                                        const mcpt_adaptive_params* ap, double* d_mean3, double* d_stderr3, int32_t* d_hits, int32_t* d_counts,
                                        mcpt_stats* stats, void* stream)
{
    if (const int rc = query_params_check(p, n, d_q6, d_mean3)) return rc;
    if (const int rc = adaptive_params_check(ap)) return rc;
    return adaptive_query_device(d, DQuery{d_q6, p->kind, d_mean3, d_stderr3, d_hits}, d_ids, n, p->spp, p->sample_base, p->seed, p->flags, *ap, d_counts,
                                 stats, stream);
}

int mcpt_query_radiance_adaptive(mcpt_device* d, const double* q6, const int32_t* ids, int64_t n, const mcpt_query_params* p,
                                 const mcpt_adaptive_params* ap, double* mean3, double* stderr3, int32_t* hits, int32_t* counts, mcpt_stats* stats)
{
    if (const int rc = query_params_check(p, n, q6, mean3)) return rc;
    if (const int rc = query_list_check(q6, ids, n, p->kind)) return rc;
    if (const int rc = adaptive_params_check(ap)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return MCPT_OK;
    const size_t sn = size_t(n);
    Staging S(d->stream.get());
    const int32_t* d_ids = nullptr;
    int32_t* d_counts = nullptr;
    DQuery q{nullptr, p->kind, nullptr, nullptr, nullptr};
    if (const int rc = S.in(q6, sn * 6, "the query list", q.q6)) return rc;
    if (const int rc = S.in(ids, sn, "the queries' ids", d_ids)) return rc;
    if (const int rc = S.out(mean3, sn * 3, "the queries' answers", q.mean3)) return rc;
    if (const int rc = S.out(stderr3, sn * 3, "the queries' standard errors", q.stderr3)) return rc;
    if (const int rc = S.out(hits, sn, "the queries' hits", q.hits)) return rc;
    if (const int rc = S.out(counts, sn, "the queries' sample counts", d_counts)) return rc;
    return S.finish(adaptive_query_device(d, q, d_ids, n, p->spp, p->sample_base, p->seed, p->flags, *ap, d_counts, stats, d->stream.get()));
}

}  // extern "C"
