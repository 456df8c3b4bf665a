// What the calls that answer a list by closest hits, chunk by chunk, share on the host (hit_work.hpp).
#include "hit_work.hpp"

#include <string>

#include "handles.hpp"

using namespace mcpt;

int hit_work_grow(HitWork& w, int64_t rays, int64_t cap_rays, const char* noun, bool own_rays)
{
    const std::string the = std::string("the ") + noun;
    if (rays > cap_rays) return fail(MCPT_ERR_NOMEM, the + " workspace of " + std::to_string(rays) + " rays cannot be allocated");
    const size_t sr = size_t(rays);
    if (own_rays)
        if (const int rc = grow(w.rays6, sr * 6, (the + " rays").c_str())) return rc;
    if (const int rc = grow(w.t, sr, (the + " rays' distances").c_str())) return rc;
    if (const int rc = grow(w.p, sr * 3, (the + " rays' hit points").c_str())) return rc;
    return grow(w.leaf, sr, (the + " rays' hits").c_str());
}

void trace_leaf(mcpt_device* d, const double* d_rays6, long long n, int32_t* d_leaf, double* d_t, double* d_p, hipStream_t st)
{
    launch_trace_closest_leaf(d->ds, d->trace_mode == MCPT_TRACE_FAST, d_rays6, n, d_leaf, d_t, d_p, d->aux_ctr.get(), d->aux_queue.get(),
                              d->aux_slow_list.get(), d->slow_cap, st, d->cfg);
}

int host_form_begin(mcpt_device* d, hipStream_t& st)
{
    st = d->stream.get();
    HIP_TRY(hipMemsetAsync(d->aux_ctr.get(), 0, sizeof(DCounters), st));
    HIP_TRY(hipEventRecord(d->ev[0].get(), st));
    return MCPT_OK;
}

int host_form_end(mcpt_device* d, Staging& S, int64_t answered, mcpt_stats* stats)
{
    int launched = launch_result();
    if (launched == MCPT_OK) {
        const hipError_t e = hipEventRecord(d->ev[1].get(), d->stream.get());
        if (e != hipSuccess) launched = fail(MCPT_ERR_HIP, std::string("hipEventRecord: ") + hipGetErrorString(e));
    }
    if (const int rc = S.finish(launched)) return rc;          // (the stream is waited for whatever came of the launch)
    if (!stats) return MCPT_OK;
    DCounters c{};
    HIP_TRY(hipMemcpy(&c, d->aux_ctr.get(), sizeof c, hipMemcpyDeviceToHost));
    counters_to_stats(c, stats, d->knobs.print_diag != 0);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, d->ev[0].get(), d->ev[1].get());
    if (answered != kNotReported) stats->rays_primary = uint64_t(answered);
    stats->ms_trace = ms; stats->ms_total = ms; stats->launches = 1;
    return MCPT_OK;
}

int chunk_stats(mcpt_stats* stats, int64_t n, int64_t rays_per_item, int chunks, hipStream_t st)
{
    if (!stats) return MCPT_OK;
    HIP_TRY(hipStreamSynchronize(st));
    stats->rays_primary = stats->samples = uint64_t(n) * uint64_t(rays_per_item);
    stats->launches = chunks;
    return MCPT_OK;
}
